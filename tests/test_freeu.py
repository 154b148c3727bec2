"""FreeU without a GPU: the closed form against the literal torch.fft transcription of diffusers' fourier_filter, the bar of the GPU test
(its accumulation allowance measured here, its power shown on six mutations), the discrimination of the forward test's settings, and the
host plumbing from --freeu down to the pipeline attribute.  The GPU side is tests/test_freeu_gpu.py; both share tests/freeu_ref.py."""
import json
import os
import pickle
import subprocess
import sys
import types

import pytest
import torch

import freeu_ref as R
from freeu_ref import FORWARD_BAR, FORWARD_FREEU, forward_case, oracle_streams, rel_l2
from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, OracleUNet, random_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------------------------------------------------------- the closed form
@pytest.mark.parametrize("grid", [(2, 2), (2, 6), (3, 5), (4, 6), (8, 12), (32, 32)])
@pytest.mark.parametrize("s", [0.2, 0.9, 1.5])
def test_closed_form_equals_the_literal_fourier_filter(grid, s):
    """The four-bin restatement is diffusers' fourier_filter(x, threshold=1, scale=s) - fftshift, box mask, ifftshift, ifftn, .real -
    to 1e-12 relative, on even, odd and 2-wide sides (where bin -1 is the Nyquist bin) alike."""
    H, W = grid
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(3, 5, H, W, generator=g, dtype=torch.float64) + torch.randn(3, 5, 1, 1, generator=g, dtype=torch.float64)
    lit, closed = R.fourier_filter_literal(x, 1, s), R.skip_ref(x, s)
    err = (lit - closed).abs().max().item() / lit.abs().max().item()
    print(f"grid {H}x{W} s {s}: closed form vs literal transcription, max error / max|out| = {err:.3e}")
    assert err <= 1e-12


def test_a_2x2_grid_is_scaled_as_a_whole():
    """On 2 x 2 the four bins are the whole spectrum: the filter multiplies the map by s (a check of the restatement against arithmetic
    one can do by hand)."""
    x = torch.randn(4, 2, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    assert torch.allclose(R.skip_ref(x, 0.3), 0.3 * x, rtol=0, atol=1e-15)


# ---------------------------------------------------------------------------------------------------------------- the bar
def _measured_inputs(H, W):
    """The skip inputs of the GPU op test on this grid, as maps [N, H, W]: all seven streams; every channel on the small grids, every
    16th on the two large ones (a subset can only give a smaller maximum, i.e. a stricter bar)."""
    sk = R.op_inputs(H, W)[1]
    if (H, W) in R.LARGE_GRIDS:
        sk = sk[:, :, ::16]
    return R.to_maps(sk, H, W).reshape(-1, H, W)


def _fp32_distance(H, W, s):
    m = _measured_inputs(H, W)
    ref = R.skip_ref(m, s)
    got = torch.from_numpy(R.skip_fp32_numpy(m.reshape(m.shape[0], -1).numpy(), H, W, s)).double().reshape(m.shape)
    unit = abs(s - 1.0) * m.double().abs().amax(dim=(-2, -1), keepdim=True)
    return ((got - ref).abs() / unit).max().item()


def test_accumulation_allowance_is_the_measured_one():
    """A of the bar is 4 x the largest distance of the fp32 numpy evaluation from fp64, before the fp16 rounding, in units of
    |s - 1| max|sk|, on the GPU test's own inputs.  Re-measured here: the constants in freeu_ref.py must be these figures (written
    rounded up to two digits: the measurement must not exceed them, and not fall below half of them)."""
    worst = 0.0
    for (H, W) in R.OP_GRIDS:
        for s in R.OP_S:
            d = _fp32_distance(H, W, s)
            print(f"grid {H}x{W} s {s}: fp32 numpy vs fp64, max distance / (|s - 1| max|sk|) = {d:.3e}")
            worst = max(worst, d)
    print(f"largest: {worst:.3e}; MEASURED_FP32_DISTANCE = {R.MEASURED_FP32_DISTANCE:.3e}, A = {R.ACCUMULATION_ALLOWANCE:.3e}")
    assert 0.5 * R.MEASURED_FP32_DISTANCE <= worst <= R.MEASURED_FP32_DISTANCE
    assert R.ACCUMULATION_ALLOWANCE == 4.0 * R.MEASURED_FP32_DISTANCE


def test_fp32_evaluation_rounded_to_fp16_meets_the_bar():
    """The bar is satisfiable: the fp32 numpy evaluation, rounded to fp16, lies inside it on every grid."""
    for (H, W) in R.OP_GRIDS:
        m = _measured_inputs(H, W)
        for s in R.OP_S:
            ref = R.skip_ref(m, s)
            got = torch.from_numpy(R.skip_fp32_numpy(m.reshape(m.shape[0], -1).numpy(), H, W, s)).half().double().reshape(m.shape)
            ratio = ((got - ref).abs() / R.bar(ref, m, s)).max().item()
            print(f"grid {H}x{W} s {s}: fp16(fp32 numpy) worst ratio to the bar {ratio:.3f}")
            assert ratio <= 1.0


SKIP_MUTATIONS = {                                     # name -> (keyword of skip_ref, the grids on which it changes the result at all)
    "+1 instead of -1 on the x axis": (dict(kx_low=+1), lambda H, W: H > 2 and W > 2),
    "missing .real halving": (dict(count_conjugate=True), lambda H, W: True),
    "H and W swapped in the twiddles": (dict(swap_hw=True), lambda H, W: H != W),
    "s instead of s - 1": (dict(s_not_minus_one=True), lambda H, W: True),
    "DC bin left out": (dict(no_dc=True), lambda H, W: True),
}


@pytest.mark.parametrize("name", list(SKIP_MUTATIONS))
def test_skip_mutations_exceed_the_bar(name):
    """Each wrong filter, evaluated in fp64 (no rounding at all in its favour), lies outside the bar on the GPU test's inputs, on every
    grid where it is a different function.  +1 on the x axis alone is the other diagonal of bins; flipping BOTH axes would give the
    conjugates of the right bins, which the real part cannot see - and with H == 2 or W == 2 (-1 == +1 there) one flip is such a
    conjugation too, so those grids are not asked.  The swap needs H != W."""
    kw, visible = SKIP_MUTATIONS[name]
    seen = 0
    for (H, W) in R.OP_GRIDS:
        if not visible(H, W):
            continue
        m = _measured_inputs(H, W)
        for s in R.OP_S:
            ref, mut = R.skip_ref(m, s), R.skip_ref(m, s, **kw)
            factor = ((mut - ref).abs() / R.bar(ref, m, s)).max().item()
            print(f"{name}: grid {H}x{W} s {s}: exceeds the bar by a factor of {factor:.1f}")
            assert factor > 2.0, (name, H, W, s)
            seen += 1
    assert seen >= 6


def test_backbone_mutation_exceeds_the_bar():
    """C1 // 2 replaced by C1: the upper half of the channels moves by |x| |b - 1|, far outside one fp16 rounding."""
    for (H, W) in R.OP_GRIDS:
        x = R.op_inputs(H, W)[0][:, :, :64]
        for b in (1.4, 0.7):
            ref, mut = R.backbone_ref(x, b), R.backbone_ref(x, b, half=64)
            factor = ((mut - ref).abs() / R.round_bar(ref)).max().item()
            print(f"C1 instead of C1 // 2: grid {H}x{W} b {b}: exceeds the bar by a factor of {factor:.1f}")
            assert factor > 2.0
            assert torch.equal(mut[..., :32], ref[..., :32])


# ---------------------------------------------------------------------------------------------------------------- discrimination
@pytest.mark.parametrize("which", ["xl", "sd"])
def test_forward_settings_discriminate(which):
    """With the settings the GPU forward test uses, FreeU moves every stream's output at least 10 x the forward bar away from the
    plain oracle: an engine that ignored rt_set_freeu - or applied it to some streams only - cannot pass that test."""
    c = forward_case(which)
    off = oracle_streams(OracleUNet(c["cfg"], c["sd"]), c)
    on = oracle_streams(R.FreeUOracleUNet(c["cfg"], c["sd"], **FORWARD_FREEU), c)
    for name, a, b in zip(("uncond", "base+fontsize", "text_ref", "region injected"), on, off):
        r = rel_l2(a, b)
        print(f"{which} stream {name}: rel-L2(FreeU oracle, plain oracle) = {r:.3e}")
        assert r >= 10 * FORWARD_BAR, name


def test_oracle_hidden_channel_split_follows_the_up_path_wiring():
    """C1 of FreeUOracleUNet against oracle/shapes.py: conv1 of up resnet (i, j) takes C1 + skip channels."""
    from oracle.shapes import weight_shapes
    for cfg in (TINY_XL_CONFIG, TINY_SD_CONFIG):
        o = R.FreeUOracleUNet(cfg, random_state_dict(cfg, seed=1), 1, 1, 1, 1)
        boc = cfg["block_out_channels"]
        skips = [boc[0]]
        for i, c in enumerate(boc):
            skips += [c] * (cfg["layers_per_block"] if isinstance(cfg["layers_per_block"], int) else cfg["layers_per_block"][i])
            if i != len(boc) - 1:
                skips.append(c)
        shapes = weight_shapes(cfg)
        for i in range(len(boc)):
            for j in range(3):
                assert shapes[f"up_blocks.{i}.resnets.{j}.conv1.weight"][1] == o._hidden_channels(i, j) + skips.pop()


# ---------------------------------------------------------------------------------------------------------------- host plumbing
def test_enable_freeu_argument_order_and_checks():
    """diffusers' order s1, s2, b1, b2, on the pipelines' mixin and on the UNet object; the engine call receives the same order."""
    from rich_text_to_image_amd.freeu import OFF, FreeUMixin, check_freeu
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    from rich_text_to_image_amd.region_diffusion_sdxl import RegionDiffusionXL
    from rich_text_to_image_amd.unet import HipUNet2DConditionModel
    assert issubclass(RegionDiffusion, FreeUMixin) and issubclass(RegionDiffusionXL, FreeUMixin)
    calls = []
    eng = types.SimpleNamespace(set_freeu=lambda *a: calls.append(a))
    p = FreeUMixin()
    p.apply_freeu(eng)
    p.enable_freeu(0.9, 0.2, 1.5, 1.6)
    assert p.freeu == (0.9, 0.2, 1.5, 1.6)
    p.apply_freeu(eng)
    p.disable_freeu()
    assert p.freeu is None
    p.apply_freeu(eng)
    assert calls == [OFF, (0.9, 0.2, 1.5, 1.6), OFF]
    for bad in ((0.0, 1, 1, 1), (1, -1, 1, 1), (1, 1, float("nan"), 1), (1, 1, 1, float("inf")), (1, 1, 1), (1, 1, 1, 1, 1), "abcd"):
        with pytest.raises(ValueError):
            check_freeu(bad)
    with pytest.raises(ValueError):
        p.enable_freeu(1, 1, 0, 1)
    assert p.freeu is None
    u = HipUNet2DConditionModel(TINY_XL_CONFIG)
    u._engines[(8, 8)] = eng
    del calls[:]
    u.enable_freeu(0.6, 0.4, 1.1, 1.2)
    assert u.freeu == (0.6, 0.4, 1.1, 1.2) and calls == [(0.6, 0.4, 1.1, 1.2)]
    p.unet = u                                    # a pipeline without a setting of its own runs with its UNet's
    p.apply_freeu(eng)
    assert calls[-1] == (0.6, 0.4, 1.1, 1.2)


def _ns(**k):
    return types.SimpleNamespace(**dict(dict(requests=None, rich_text_json=None, seeds=None, seed=6, negative_prompt="", freeu=None), **k))


def test_freeu_flag_and_requests_key_reach_the_requests(tmp_path):
    from rich_text_to_image_amd.sample import build_parser, build_requests, check_freeu_arg
    j = '{"ops":[{"insert":"a cat\\n"}]}'
    a = build_parser().parse_args(["--rich_text_json", j, "--freeu", "0.9", "0.2", "1.5", "1.6"])
    a.freeu = check_freeu_arg(a.freeu, "--freeu")
    assert build_requests(a)[0]["freeu"] == [0.9, 0.2, 1.5, 1.6]
    assert build_requests(build_parser().parse_args(["--rich_text_json", j]))[0]["freeu"] is None
    f = tmp_path / "reqs.jsonl"
    f.write_text(json.dumps({"rich_text_json": json.loads(j), "freeu": [0.6, 0.4, 1.1, 1.2]}) + "\n" + json.dumps({"rich_text_json": json.loads(j)}) + "\n")
    r = build_requests(_ns(requests=str(f), freeu=[0.9, 0.2, 1.5, 1.6]))
    assert r[0]["freeu"] == [0.6, 0.4, 1.1, 1.2] and r[1]["freeu"] == [0.9, 0.2, 1.5, 1.6]      # a line's own, else the flag's


def test_generate_sets_the_pipeline_attribute_and_restores_it(monkeypatch):
    """param['freeu'] is the pipeline attribute for the duration of the request - also when the request fails - and the earlier setting
    comes back after it, the way guidance_rescale does."""
    from rich_text_to_image_amd import sample
    from rich_text_to_image_amd.freeu import FreeUMixin
    seen = []

    def body(model, param, *a):
        seen.append((model.freeu, "freeu" in param and param["freeu"]))
        if param.get("boom"):
            raise RuntimeError("boom")
        return "plain", "rich", {}
    monkeypatch.setattr(sample, "_generate", body)
    m = FreeUMixin()
    sample.generate(m, {"freeu": [0.9, 0.2, 1.5, 1.6]})
    assert seen[-1][0] == (0.9, 0.2, 1.5, 1.6) and m.freeu is None
    m.enable_freeu(0.6, 0.4, 1.1, 1.2)
    sample.generate(m, {"freeu": None})
    assert seen[-1][0] == (0.6, 0.4, 1.1, 1.2)                      # no key / None: the pipeline as it is
    with pytest.raises(RuntimeError):
        sample.generate(m, {"freeu": (0.9, 0.2, 1.5, 1.6), "boom": True})
    assert seen[-1][0] == (0.9, 0.2, 1.5, 1.6) and m.freeu == (0.6, 0.4, 1.1, 1.2)
    with pytest.raises(ValueError):
        sample.generate(m, {"freeu": [1, 1, 1]})
    assert m.freeu == (0.6, 0.4, 1.1, 1.2)


@pytest.mark.parametrize("argv", [["--freeu", "0", "1", "1", "1"], ["--freeu", "1", "1", "nan", "1"], ["--freeu", "1", "1", "1", "inf"],
                                  ["--freeu", "1", "-2", "1", "1"], ["--freeu", "1", "1", "1"], ["--requests", "BAD"]])
def test_bad_freeu_values_are_refused_before_any_rank_starts(argv, tmp_path, monkeypatch):
    from rich_text_to_image_amd import launcher, sample

    def never(*a, **k):
        raise AssertionError("the launch was reached")
    monkeypatch.setattr(launcher, "self_launch", never)
    monkeypatch.setattr(launcher, "init_distributed", never)
    j = '{"ops":[{"insert":"a cat\\n"}]}'
    if argv[0] == "--requests":
        f = tmp_path / "reqs.jsonl"
        f.write_text(json.dumps({"rich_text_json": json.loads(j)}) + "\n" + json.dumps({"rich_text_json": json.loads(j), "freeu": [1, 1, 0]}) + "\n")
        argv = ["--requests", str(f)]
    with pytest.raises(SystemExit) as e:
        sample.main(["--rich_text_json", j, "--gpus", "2"] + argv)
    assert e.value.code not in (0, None)


def test_settings_survive_the_pipeline_broadcast_serialisation():
    """launcher.broadcast_pipeline ships pipeline_settings() of the source rank as a pickled object and applies it on the others."""
    from rich_text_to_image_amd.freeu import FreeUMixin
    from rich_text_to_image_amd.launcher import apply_pipeline_settings, pipeline_settings
    src, dst = FreeUMixin(), FreeUMixin()
    src.enable_freeu(0.9, 0.2, 1.5, 1.6)
    dst.enable_freeu(0.5, 0.5, 2.0, 2.0)
    apply_pipeline_settings(dst, pickle.loads(pickle.dumps(pipeline_settings(src))))
    assert dst.freeu == (0.9, 0.2, 1.5, 1.6)
    src.disable_freeu()
    apply_pipeline_settings(dst, pickle.loads(pickle.dumps(pipeline_settings(src))))
    assert dst.freeu is None


def test_freeu_travels_with_broadcast_pipeline_to_every_rank(tmp_path):
    """Two ranks over gloo (--dry_launch: no GPU, no checkpoint): rank 0 alone sets the flag's values on its pipeline, the call
    build_model makes - launcher.broadcast_pipeline(..., pipeline=model) - leaves them on rank 1, and the three weight collectives are
    still three."""
    a = tmp_path / "a.json"
    a.write_text(json.dumps({"ops": [{"insert": "a night sky\n"}]}))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-m", "rich_text_to_image_amd.sample", "--model", "SDXL", "--gpus", "2", "--dry_launch",
                          "--rich_text_json", str(a), "--seeds", "0", "1", "--freeu", "0.6", "0.4", "1.1", "1.2"], env=env,
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert sorted(l["rank"] for l in lines) == [0, 1]
    assert all(l["freeu"] == [0.6, 0.4, 1.1, 1.2] and l["pipeline_received"] and l["broadcast_collectives"] == 3 for l in lines)
