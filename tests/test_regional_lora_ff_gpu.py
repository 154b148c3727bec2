"""Regional LoRA on the feed-forward, proj_in and proj_out on the GPU (csrc/lora.hip: lora_geglu_kernel / rt_op_lora_geglu; rt_config.lora_targets
= 1): the op against the fp64 restatement of tests/regional_lora_ff_ref.py at its bar inside guarded / poisoned windows, forwards and
steps with adapters on all twelve module kinds against the merged oracle, and off is off."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import regional_lora_ff_ref as F  # noqa: E402
import regional_lora_ref as R  # noqa: E402
from freeu_ref import FORWARD_BAR, rel_l2  # noqa: E402
from memguard import PATTERN, damage, guarded, intact, poisoned  # noqa: E402
from test_regional_lora_gpu import (GOLDEN, SLOT_SCALES, STEP_BAR, STEP_GS, _bits, _engine, _forward, _lora_case, _oracle_forward,  # noqa: E402
                                    _rich_reset, _set_prompts)

DEV = "cuda:0"
LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "regional_lora_ff_gpu_tests.log")
_logged = []


def _log(line):
    """Prints the figure and keeps it in profiles/regional_lora_ff_gpu_tests.log (rewritten by every run of this module)."""
    print(line)
    _logged.append(line)
    try:
        with open(LOG, "w") as f:
            f.write("\n".join(_logged) + "\n")
    except OSError:
        pass


def _launch(inp, streams=None, pad=8):
    """rt_op_lora_geglu on the inputs of geglu_inputs, every operand in a guarded / poisoned window with leading dimensions `pad` larger than
    the packed widths.  -> (out [B', rows, N / 2] on the CPU, launched entries, (big, window) of out)."""
    from rich_text_to_image_amd.engine import lora_geglu
    X, Z = inp["X"], inp["Z"]
    streams = list(range(X.shape[0])) if streams is None else streams
    B, rows, K, N = len(streams), X.shape[1], X.shape[2], Z.shape[2]
    xd = poisoned(X[streams].reshape(B * rows, K).to(DEV), K + pad)
    zd = poisoned(Z[streams].reshape(B * rows, N).to(DEV), N + pad)
    dd, ud = poisoned(inp["down"].to(DEV), K + pad), poisoned(inp["up"].to(DEV), inp["up"].shape[1] + pad)
    ad, cd = poisoned(inp["aor"].to(DEV)), poisoned(inp["col"].to(DEV))
    big, od = guarded((B * rows, N // 2), torch.bfloat16, N // 2 + pad, fill="bytes", device=DEV)
    n = lora_geglu(xd, dd, ud, ad, cd, zd, od, [b * rows for b in range(B)], [inp["scales"][s] for s in streams], rows)
    return od.cpu().reshape(B, rows, N // 2), n, (big, od)


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == PATTERN).all())


@pytest.mark.parametrize("case", F.GEGLU_CASES, ids=F.GEGLU_IDS)
def test_op_matches_the_fp64_restatement(case):
    """Every element of every adapted stream within the bar of (Zv + Dv) gelu(Zg + Dg) in fp64; the rows of streams with all-zero scales
    are not written and those streams are not in the grid; guards and padding columns of out stay intact and the poison around every
    input is never read; a second launch gives the same bits."""
    inp = F.geglu_inputs(case)
    got, n, (big, od) = _launch(inp)
    ref, bar = F.geglu_ref(inp, acc_units=F.GPU_GEGLU_ACC_UNITS)
    adapted = [b for b, s in enumerate(inp["scales"]) if any(s)]
    worst, share = R.worst_and_share(got[adapted], ref[adapted], bar[adapted])
    zv, zg = F.split_packed(inp["Z"])
    far, _ = R.worst_and_share(F.bf(zv * F.gelu_poly(zg))[adapted], ref[adapted], bar[adapted])
    _log(f"lora_geglu {case['name']} (streams {len(case['scales'])}, rows {case['rows']}, K {case['K']}, N {case['N']}, ranks {case['ranks']}): "
         f"worst |got - ref| / bar = {worst:.3f}; the base projection alone (no term) is at {far:.1f}")
    assert n == len(adapted)
    assert intact(big, od), damage(big, od)
    assert bool(torch.isfinite(got[adapted].float()).all())
    assert worst <= 1.0, share
    assert far > 50.0, far
    for b in range(len(inp["scales"])):
        assert b in adapted or _untouched(got[b]), b
    again, _, _ = _launch(inp)
    assert torch.equal(_bits(again), _bits(got))


@pytest.mark.parametrize("case", F.GEGLU_CASES[1:], ids=F.GEGLU_IDS[1:])
def test_op_is_batch_invariant(case):
    """An adapted stream launched alone, at row offset 0, equals the same stream inside the full launch, bit for bit."""
    inp = F.geglu_inputs(case)
    full, _, _ = _launch(inp)
    for b, s in enumerate(inp["scales"]):
        if any(s):
            one, n, _ = _launch(inp, streams=[b], pad=24)
            assert n == 1 and torch.equal(_bits(one[0]), _bits(full[b])), b


def test_op_launches_and_writes_nothing_without_an_adapted_stream():
    inp = F.geglu_inputs(F.GEGLU_CASES[0])
    inp["scales"] = [[0.0] * 4]
    got, n, (big, od) = _launch(inp)
    assert n == 0 and _untouched(got) and intact(big, od)


def test_op_refuses_what_it_cannot_do():
    """Each refusal returns RT_E_INVALID and the next call runs."""
    import ctypes as C
    from rich_text_to_image_amd.engine import RtError, lora_geglu, load_library
    inp = F.geglu_inputs(F.GEGLU_CASES[0])

    def call(rows=8, R_=16, N=64, scales=((1.0,),), rows_at=(0,), skew=0):
        X, Z = inp["X"][0].to(DEV), torch.zeros(8, N + 8, device=DEV)[:, skew:N + skew]
        down, up = torch.zeros(R_, 32, dtype=torch.bfloat16, device=DEV), torch.zeros(N, R_, dtype=torch.bfloat16, device=DEV)
        out = torch.zeros(8, N // 2, dtype=torch.bfloat16, device=DEV)
        return lora_geglu(X, down, up, torch.zeros(R_, device=DEV), torch.zeros(R_, dtype=torch.int32, device=DEV), Z, out, list(rows_at), list(scales), rows)
    assert call() == 1
    for kw in (dict(R_=8), dict(R_=144), dict(R_=24), dict(rows=4), dict(N=96), dict(skew=1), dict(scales=((float("nan"),),)),
               dict(rows_at=(0,) * 17, scales=((1.0,),) * 17)):
        with pytest.raises(RtError) as e:
            call(**kw)
        assert e.value.code == -1, kw
        assert call() == 1
    z = C.c_void_p(0)
    assert load_library().rt_op_lora_geglu(z, 32, z, 32, z, 16, z, z, z, 64, z, 32, (C.c_int * 1)(0), (C.c_float * 4)(1, 0, 0, 0), 1, 8, 32, 64, 16, None, z) == -1
    assert call() == 1


# ---------------------------------------------------------------------------------------------------------------- the engine
def _parsed(sd, cks):
    from rich_text_to_image_amd.regional_lora import parse_adapter
    return {n: parse_adapter(sd, ck, targets="transformer")[0] for n, ck in zip("AB", cks)}


@pytest.mark.parametrize("which", ["sd", "xl"])
def test_forward_with_all_twelve_module_kinds_matches_the_merged_oracle(which):
    """The six streams of test_forward_with_stream_modes_matches_the_merged_oracle with adapters on attention, feed-forward, proj_in and
    proj_out (1x1 convolutions on the SD config): every stream within the forward bar of the oracle on that stream's merged weights and
    farther than the bar from the oracle merged on the attention modules only; the scale-0 stream equals the forward of an engine
    without adapters bit for bit."""
    sd, cks, attn = F.full_adapters(which)
    c = _lora_case(which)
    off = _engine(c["cfg"], c["h"], c["w"], sd)
    eng = _engine(c["cfg"], c["h"], c["w"], sd, lora_rank=32, lora_targets=1)
    try:
        _set_prompts(off, c)
        plain = _forward(off, c)
        assert eng.bind_regional_loras(_parsed(sd, cks)) == ["A", "B"]
        _set_prompts(eng, c)
        assert torch.equal(_forward(eng, c), plain)
        eng.set_lora_scales(SLOT_SCALES)
        got = _forward(eng, c)
        eng.set_lora_scales([(0.0, 0.0)] * 4)
        assert torch.equal(_forward(eng, c), plain)
    finally:
        eng.close(); off.close()
    ref, part = _oracle_forward(c, sd, cks, SLOT_SCALES), _oracle_forward(c, sd, attn, SLOT_SCALES)
    for k, name in enumerate(("uncond", "base A 0.7", "text_ref A 0.7", "region B 1.0", "region A 0.5 + B 0.8", "injected region B 1.0")):
        r, d = rel_l2(got[k], ref[k]), rel_l2(got[k], part[k])
        _log(f"forward {which} stream {name}: rel-L2 vs the merged oracle {r:.3e}; vs the oracle merged on attention only {d:.3e}")
        assert r < FORWARD_BAR, name
        if k == 0:
            assert torch.equal(got[0], plain[0])
        else:
            assert d > FORWARD_BAR, name


def test_last_block_at_a_folded_width():
    """weight_influence_ref.FOLD_CONFIG (640 and 1280 channels, one transformer block each - the LAST of its transformer, so proj_out reads
    the bf16 trunk an emitting ff.net.2 left and the adapted rows of it are refreshed) on the 40 x 32 latent: one adapted stream between
    two that are not.  The adapted stream against the fp32 oracle on merged weights; its neighbours keep the bits of a forward without
    adapters; alone it gives its bits in the batch."""
    from oracle.unet import random_state_dict
    from weight_influence_ref import FOLD_CONFIG, FOLD_LATENT
    cfg, (h, w) = FOLD_CONFIG, FOLD_LATENT
    sd = random_state_dict(cfg, seed=4)
    ckA, _ = R.synthetic_adapter(sd, rank=4, alpha=2.0, seed=1, gain=2.0, extra=F.wide_modules(sd))
    ckB, _ = R.synthetic_adapter(sd, rank=8, seed=2, layout="peft", extra=F.wide_modules(sd))
    attn = [F.attention_part(ckA, sd), F.attention_part(ckB, sd)]
    g = torch.Generator().manual_seed(8)
    emb = torch.randn(3, 77, cfg["cross_attention_dim"], generator=g)
    lat = torch.randn(1, 4, h, w, generator=g)
    sc = [(0.0, 0.0), (0.5, 0.8), (0.0, 0.0)]
    eng = _engine(cfg, h, w, sd, lora_rank=32, lora_targets=1, max_streams=4, max_prompts=4)
    try:
        eng.bind_regional_loras(_parsed(sd, [ckA, ckB]))
        eng.set_prompts(emb.to(DEV))
        x = torch.cat([lat] * 3).to(DEV)
        plain = eng.unet_forward(x, 500.0, [0, 1, 2]).cpu()
        eng.set_lora_scales(sc)
        got = eng.unet_forward(x, 500.0, [0, 1, 2]).cpu()
        alone = eng.unet_forward(lat.to(DEV), 500.0, [1]).cpu()
    finally:
        eng.close()
    with torch.no_grad():
        ref = R.lora_oracle(cfg, sd, [ckA, ckB], sc[1:2]).forward(lat, 500.0, emb[1:2])[0]
        part = R.lora_oracle(cfg, sd, attn, sc[1:2]).forward(lat, 500.0, emb[1:2])[0]
    assert torch.equal(got[0], plain[0]) and torch.equal(got[2], plain[2]) and torch.equal(alone[0], got[1])
    r, d = rel_l2(got[1], ref), rel_l2(got[1], part)
    _log(f"folded 640 / 1280-wide last blocks, adapted stream between two others: rel-L2 vs the merged oracle {r:.3e}; vs the oracle merged on attention only {d:.3e}")
    assert r < FORWARD_BAR and d > FORWARD_BAR


# ---------------------------------------------------------------------------------------------------------------- steps
def _rich_case():
    from controlnet_ref import rich_case
    c = dict(rich_case())
    c["gs"] = STEP_GS
    wide = F.wide_modules(c["sd"])
    ckA, _ = R.synthetic_adapter(c["sd"], rank=4, alpha=2.0, seed=1, layout="kohya", gain=F.GAIN_A, extra=wide)
    ckB, _ = R.synthetic_adapter(c["sd"], rank=8, seed=2, layout="diffusers", gain=F.GAIN_B, extra=wide)
    c["cks"], c["adapters"] = [ckA, ckB], _parsed(c["sd"], [ckA, ckB])
    c["attn"] = [F.attention_part(ckA, c["sd"]), F.attention_part(ckB, c["sd"])]
    return c


@pytest.fixture(scope="module")
def rich():
    c = _rich_case()
    eng = _engine(c["cfg"], c["hw"], c["hw"], c["sd"], lora_rank=32, lora_targets=1)
    eng.bind_regional_loras(c["adapters"])
    eng.set_prompts(c["emb"].to(DEV), c["pooled"].to(DEV), c["tid"])
    eng.set_masks(c["masks"].to(DEV))
    eng.set_fontsize(torch.tensor([3, 5]), torch.tensor([4.0, -2.0]))
    eng.set_lora_scales(SLOT_SCALES)
    yield c, eng
    eng.close()


def test_region_step_matches_the_composition_of_merged_oracle_forwards(rich):
    """The injected first region_step with the base on adapter A, region 0 on B and region 1 on both, all twelve module kinds adapted:
    both latent streams against rich_step_forwards on the oracle with each forward's merged weights, on the latent UPDATE."""
    from oracle.region_loop import rich_step_forwards
    c, eng = rich
    R_ = c["masks"].shape[0]
    _rich_reset(eng, c)
    eng.region_step(0, c["gs"], c["isa"], 0.0, xl=True)
    got, got_ref = (t.cpu() for t in eng.read_latents(c["hw"], c["hw"], with_ref=True))
    sched, lat0, gs = c["sched"], c["lat"], c["gs"]
    t = sched.timesteps[0]
    slots = [0, R_, 0, R_] + list(range(1, R_))

    def added_fn(k):
        k = k if k >= 0 else c["pooled"].shape[0] + k
        return {"text_embeds": c["pooled"][k:k + 1], "time_ids": c["tid"]}
    lat_in = sched.scale_model_input(lat0, t)
    tfd = {"word_pos": torch.tensor([3, 5]), "font_size": torch.tensor([4.0, -2.0])}
    masks = [c["masks"][r:r + 1] for r in range(R_)]

    def compose(cks):
        unet = R.lora_oracle(c["cfg"], c["sd"], cks, [SLOT_SCALES[s] for s in slots])
        eu, et, eur, etr = rich_step_forwards(unet, lat_in, lat_in.clone(), t, c["emb"], added_fn, masks, tfd, True, True)
        out = sched.step(torch.cat([eu + gs * (et - eu), eur + gs * (etr - eur)]), t, torch.cat([lat0, lat0]))["prev_sample"]
        return torch.chunk(out, 2, dim=0)
    (ref, ref_ref), (pt, pt_ref) = compose(c["cks"]), compose(c["attn"])
    r, rr = rel_l2(got - lat0, ref - lat0), rel_l2(got_ref - lat0, ref_ref - lat0)
    d, dr = rel_l2(pt - lat0, ref - lat0), rel_l2(pt_ref - lat0, ref_ref - lat0)
    _log(f"region_step, adapters on twelve module kinds: latent UPDATE rel-L2 {r:.3e} (reference stream {rr:.3e}); the oracle merged on attention only is {d:.3e} / {dr:.3e} away")
    assert r < STEP_BAR and rr < STEP_BAR
    assert d > STEP_BAR and dr > STEP_BAR


def test_plain_step_matches_the_composition_of_merged_oracle_forwards():
    """plain_step (streams [uncond = slot 0, text = slot 1]) with adapter A at 0.7 and B at 0.4 on the text prompt only."""
    c = _rich_case()
    eng = _engine(c["cfg"], c["hw"], c["hw"], c["sd"], lora_rank=32, lora_targets=1)
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

    def compose(cks):
        unet = R.lora_oracle(c["cfg"], c["sd"], cks, sc)
        with torch.no_grad():
            eu = unet.forward(x, t, emb[:1], {"text_embeds": pooled[:1], "time_ids": c["tid"]})
            et = unet.forward(x, t, emb[1:], {"text_embeds": pooled[1:], "time_ids": c["tid"]})
        return sched.step(eu + gs * (et - eu), t, lat0)["prev_sample"]
    ref, pt = compose(c["cks"]), compose(c["attn"])
    r, d = rel_l2(got - lat0, ref - lat0), rel_l2(pt - lat0, ref - lat0)
    _log(f"plain_step, adapters on twelve module kinds: latent UPDATE rel-L2 {r:.3e}; the oracle merged on attention only is {d:.3e} away")
    assert r < STEP_BAR
    assert d > STEP_BAR


def test_split_step_equals_the_whole_step(rich):
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


def test_region_step_is_hipgraph_capturable(rich):
    """Nothing is allocated inside the step - the fp32 scratch of the unfused ff.net.0.proj and its GEMM's split-K scratch were planned by
    the dry forward -: the replay of a captured step gives the eager step's bits."""
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


def test_the_new_launches_are_profiled_as_lora(rich):
    """Per transformer block the six attention launches, ff.net.2's and one lora_geglu launch per adapted stream; per transformer proj_in's
    and proj_out's."""
    import ctypes as C
    c, eng = rich
    R_ = c["masks"].shape[0]
    adapted = sum(any(SLOT_SCALES[s]) for s in [0, R_, 0, R_] + list(range(1, R_)))
    _rich_reset(eng, c)
    eng.profile_enable(True)
    eng.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True)
    eng.synchronize()
    n, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
    assert eng.lib.rt_profile_read2(eng.h, 9, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)) == 0
    eng.profile_enable(False)
    blocks = eng.lib.rt_attn_module_count(eng.h) // 2
    transformers = len([k for k in c["sd"] if k.endswith(".proj_in.weight")])
    assert n.value == (7 + adapted) * blocks + 2 * transformers and by.value > 0 and ms.value > 0, (n.value, blocks, transformers, adapted)


# ---------------------------------------------------------------------------------------------------------------- off is off
def test_off_is_off_with_the_wide_engine():
    """An engine with lora_targets = 1, adapters bound and every scale 0 - and the same engine after scales were set and cleared -
    reproduces the digests of tests/golden/regional_lora_off_bits.json, recorded before regional LoRA existed."""
    from controlnet_ref import off_digests
    with open(GOLDEN) as f:
        want = json.load(f)["digests"]

    def wide(cfg, h, w, sd):
        e = _engine(cfg, h, w, sd, lora_rank=32, lora_targets=1)
        ck, _ = R.synthetic_adapter(sd, rank=4, alpha=2.0, seed=1, gain=2.0, extra=F.wide_modules(sd))
        e.bind_regional_loras(_parsed(sd, [ck]))
        return e

    def set_and_clear(eng, c):
        P = c["emb"].shape[0]
        eng.set_lora_scales([(0.9,)] * P)
        eng.set_lora_scales([(0.0,)] * P)
    assert off_digests(wide, lambda eng, c: eng.set_lora_scales([(0.0,)] * c["emb"].shape[0])) == want
    assert off_digests(wide, set_and_clear) == want


def test_an_attention_file_runs_the_same_bits_under_either_targets():
    from rich_text_to_image_amd.unet import HipUNet2DConditionModel
    sd, cks, attn = F.full_adapters("xl")
    c = _lora_case("xl")
    outs = []
    for targets in ("attention", "transformer"):
        u = HipUNet2DConditionModel(c["cfg"], sd)
        u.load_regional_loras({"A": attn[0], "B": attn[1]}, targets=targets)
        eng = u.engine(c["h"], c["w"])
        try:
            assert eng.lora_targets == 0
            _set_prompts(eng, c)
            eng.set_lora_scales(SLOT_SCALES)
            outs.append(_forward(eng, c))
        finally:
            eng.close()
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------- facade and CLI
def test_facade_and_cli_round_trip(tmp_path):
    """A synthetic full adapter (kohya layout, all twelve module kinds, written by tools/make_regional_lora.py --targets transformer):
    load_regional_loras(targets="transformer") applies every module and builds the wide engine; python -m rich_text_to_image_amd.sample
    --region_lora x.safetensors:0 --region_lora_targets transformer runs it, and its rich pass differs from the run that drops the four
    modules; without the flag the file is refused by name."""
    import sys
    from rich_text_to_image_amd import sample
    from rich_text_to_image_amd.region_diffusion_sdxl import RegionDiffusionXL
    from oracle.unet import TINY_XL_CONFIG
    from test_checkpoint_gpu import _write_dir
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_regional_lora
    _write_dir(str(tmp_path / "ckpt"))
    a = str(tmp_path / "full_kohya.safetensors")
    make_regional_lora.main([a, "--config", "sd", "--rank", "4", "--alpha", "2", "--layout", "kohya", "--seed", "1", "--targets", "transformer"])
    sd, cks, _ = F.full_adapters("xl")
    m = RegionDiffusionXL(device=0, unet_state_dict=sd, config=TINY_XL_CONFIG)
    rep = m.load_regional_loras({"x": cks[0]}, targets="transformer")
    assert sorted(rep["x"]["applied"]) == sorted(R.attention_projections(sd) + F.wide_modules(sd)) and rep["x"]["dropped"] == []
    assert (m.unet.lora_rank, m.unet.lora_targets) == (16, 1)
    with pytest.raises(ValueError, match="ff.net.0.proj"):
        m.load_regional_loras({"x": cks[0]})
    js = json.dumps({"ops": [{"insert": "a "}, {"attributes": {"link": "a wooden fence covered in snow"}, "insert": "fence"},
                             {"insert": " under a night sky\n"}]})
    common = ["--load_path", str(tmp_path / "ckpt"), "--model", "SD", "--sample_steps", "12", "--seed", "3", "--num_segments", "4", "--inject_selfattn", "0.2",
              "--rich_text_json", js, "--region_lora", f"{a}:0"]
    _, dropped = sample.main(common + ["--run_dir", str(tmp_path / "out0"), "--region_lora_attention_only"])
    _, rich_ = sample.main(common + ["--run_dir", str(tmp_path / "out"), "--region_lora_targets", "transformer"])
    assert rich_.shape == dropped.shape == (1, 512, 512, 3) and (rich_ != dropped).any()
    with pytest.raises(SystemExit, match="ff.net.0.proj"):
        sample.main(common + ["--run_dir", str(tmp_path / "out1")])
