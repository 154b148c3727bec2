"""CPU: the fp64 restatement of the guided-prediction pre-pass (tests/guided_ref.py) that tests/test_guided_prediction_gpu.py holds
csrc/guided.hip to, and the host side of v-prediction / guidance_rescale: scheduler keywords, trailing spacing, the command line and the
checkpoint's scheduler_config.json.

The restated rescale is pinned to the reference's own rescale_noise_cfg; the three solvers restated there with magnitudes are pinned to
tests/dpm_solver_ref.py / tests/sde_ref.py; the v route fed v = (eps - cx x) / cv reproduces the eps route of those pinned restatements;
and every named mutation moves a one-step output of the GPU matrix far beyond the GPU bar.

`biased_std` is the exception the arithmetic forces: the factor is phi std_text / std_cfg + (1 - phi), and n instead of n - 1 in BOTH
standard deviations multiplies numerator and denominator by the same sqrt((n - 1) / n): the ratio, hence every output, is unchanged
(measured: <= 1e-3 of the bar, fp64 noise).  That variant is no bug, and the test says so; the one-sided `biased_std_cfg` is the variant
that is one; it moves the factor by 1 / (2n) relative only and is held to >= 20 x the bar, the others to >= 100 x."""
import json

import numpy as np
import pytest
import torch

from oracle import refload
from tests import guided_ref as G
from tests import step_ref as S
from tests.dpm_solver_ref import RefDPMSolver
from tests.sde_ref import RefEulerAncestral, RefSdeDpmSolver, field_fn


def _field(case):
    h, w = case["lat"]
    return field_fn(41, h, w)


# ------------------------------------------------------------------------------------------------ the restatement
def test_mutations_are_caught_by_the_gpu_bar():
    margins = {}
    for m in G.MUTATIONS:
        margins[m] = max(G.one_step_margins(c, (m,), _field(c)) for c in G.CASES)
        print(f"mutation {m}: worst one-step change {margins[m]:.3g} x the bar")
    invariant = margins.pop("biased_std")
    assert invariant <= 1e-3, invariant                     # a ratio of two standard deviations with the same n: see the module docstring
    # one-sided: the factor's phi part moves by 1 / (2n) relative, n = 384 values on the 12 x 8 grid: about phi r / (2 n f) >= 2e-4 of
    # the prediction, against a bar of 16 u (magnitude / value) <= 1e-5 of it - at least 20 bars, not the 100 of a structural mistake
    assert margins.pop("biased_std_cfg") >= 20
    assert all(v >= 100 for v in margins.values()), margins
    assert G.one_step_margins(G.CASES[0], (), _field(G.CASES[0])) == 0.0


@pytest.mark.skipif(not refload.reference_available(), reason="reference tree not present")
@pytest.mark.parametrize("phi", [0.3, 0.7, 1.0])
def test_rescale_against_the_reference(phi):
    """rescale_noise_cfg of the unmodified reference, fp64, 4 x 24 x 40, g = 7.5: relative 1e-12 (n 2^-53 = 4e-13 for n = 3840 summands
    of the same formula)."""
    ref = refload.load_reference()["region_diffusion_sdxl"].rescale_noise_cfg
    g = torch.Generator().manual_seed(5)
    eu, et = (torch.randn(1, 4, 24, 40, generator=g, dtype=torch.float64) for _ in range(2))
    cfg = eu + 7.5 * (et - eu)
    want = ref(cfg, et, guidance_rescale=phi)
    got, f = G.guide(S.exact(et), S.exact(cfg), None, phi, False, None)
    rel = (got[0] - want).abs().max().item() / want.abs().max().item()
    print(f"phi {phi}: factor {f.v:.6f}, restated rescale vs rescale_noise_cfg rel {rel:.2e}")
    assert rel <= 1e-12, rel


def _pinned(kind, n, field):
    """The pinned fp64 restatement of a solver kind as step(i, eps, x) -> x'."""
    if kind in ("plms", "euler"):
        s = S.make_sched(kind, n)
        return s, lambda i, e, x: s.step(i, S.exact(e), x)[0]
    r = {"dpm2": lambda: RefDPMSolver(2, torch.float64), "sde2": lambda: RefSdeDpmSolver(field, 2, torch.float64),
         "euler_a": lambda: RefEulerAncestral(field, torch.float64)}[kind]().set_timesteps(n)
    return r, lambda i, e, x: r.step(e, r.timesteps[i], x)["prev_sample"]


@pytest.mark.parametrize("kind", list(G.KINDS))
@pytest.mark.parametrize("n", [6, 9, 20])
def test_v_route_reproduces_the_eps_route_of_the_pinned_restatement(kind, n):
    """fp64, plain steps, g = 7.5: the eps route (v off) equals the pinned solver fed the CFG-combined eps - which pins the solvers
    restated in guided_ref.py -, and the v route fed v = (eps - cx x) / cv equals it too.  1e-12."""
    h, w, g = 12, 8, 7.5
    field = field_fn(3, h, w)
    gen = torch.Generator().manual_seed(n)
    pin_s, pin = _pinned(kind, n, field)
    se, sv = G.make_sched(kind, n, noise_fn=field), G.make_sched(kind, n, noise_fn=field)
    x = torch.randn(1, 4, h, w, generator=gen, dtype=torch.float64) * G.init_sigma(kind, se)
    xp, xe, xv, worst = x, x, x, 0.0
    assert [float(t) for t in se.timesteps] == [float(t) for t in pin_s.timesteps]
    for i in range(len(se.timesteps)):
        eu, et = (torch.randn(1, 4, h, w, generator=gen, dtype=torch.float64) for _ in range(2))
        xp = pin(i, eu + g * (et - eu), xp)
        xe = G.plain_step(kind, se, i, eu, et, xe, g)["lat"][0]
        cv, cx = G.v_scalars(kind, sv, i)
        xv = G.plain_step(kind, sv, i, (eu - cx.v * xv) / cv.v, (et - cx.v * xv) / cv.v, xv, g, vpred=True)["lat"][0]
        scale = xp.abs().max().item()
        worst = max(worst, (xe - xp).abs().max().item() / scale, (xv - xp).abs().max().item() / scale)
    print(f"{kind} n={n}: worst relative distance from the pinned restatement {worst:.2e}")
    assert worst <= 1e-12, worst


def test_the_pair_is_the_plain_pass():
    """fp64: the reference pair of a rich step fed the plain step's (u, t) lands where the plain step lands, factor included."""
    c = G.CASE["dpm2_rich_v_phi"]
    x, M, steps = G.case_inputs(c)
    x, M = x.double(), [m.double() for m in M]
    rich, plain = G.make_sched("dpm2", c["n"]), G.make_sched("dpm2", c["n"])
    lat, lat_ref, p = x, x.clone(), x.clone()
    for i, ep in enumerate(steps):
        ep = {k: v.double() for k, v in ep.items()}
        r = G.step_once(c, rich, i, ep, M, lat, lat_ref)
        q = G.plain_step("dpm2", plain, i, ep["ur"], ep["tr"], p, c["g"], phi=G.phi32(c["phi"]), vpred=True)
        lat, lat_ref, p = r["lat"][0], r["lat_ref"][0], q["lat"][0]
        assert r["step_ref"] and torch.equal(lat_ref, p) and r["factor_ref"].v == q["factor"].v and r["factor"].v != q["factor"].v, i


@pytest.mark.parametrize("name", [c["name"] for c in G.CASES if c["n"] <= 8 and c["kind"] in ("plms", "euler", "dpm2")])
def test_an_fp32_evaluation_stays_within_the_bar(name):
    """The restatement evaluated on fp32 tensors from fp32 states stays within half the one-step bar of its fp64 evaluation: the bar
    (with the factor's magnitude term) is attainable."""
    c = G.CASE[name]
    x, M, steps = G.case_inputs(c)
    s32, s64 = G.make_sched(c["kind"], c["n"]), G.make_sched(c["kind"], c["n"])
    lat, lat_ref, worst = x, x.clone(), 0.0
    for i, ep in enumerate(steps):
        a = G.step_once(c, s32, i, ep, M, lat, lat_ref)
        b = G.step_once(c, s64, i, {k: v.double() for k, v in ep.items()}, [m.double() for m in M], lat.double(), lat_ref.double())
        for k in ("lat", "lat_ref", "noise_pred"):
            if k in b:
                worst = max(worst, ((a[k][0].double() - b[k][0]).abs() / (S.ULPS * S.U32 * b[k][1])).max().item())
        lat = a["lat"][0].float()
        lat_ref = a["lat_ref"][0].float() if "lat_ref" in a else lat_ref
    print(f"{name}: fp32 evaluation worst error / bar {worst:.3f}")
    assert worst < 0.5, worst


# ------------------------------------------------------------------------------------------------ tables
def test_trailing_lists_are_pinned():
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerAncestralTables, EulerTables, trailing_timesteps
    assert trailing_timesteps(4).tolist() == [999, 749, 499, 249]
    assert trailing_timesteps(1000).tolist() == list(range(999, -1, -1))
    for mk in (lambda: DPMSolverTables(timestep_spacing="trailing"), lambda: DPMSolverTables(1, algorithm="sde-dpmsolver++", timestep_spacing="trailing")):
        assert mk().set_timesteps(4).timesteps.tolist() == [999, 749, 499, 249]
        assert mk().set_timesteps(1000).timesteps.tolist() == list(range(999, -1, -1))
    for cls in (EulerTables, EulerAncestralTables):
        t = cls(timestep_spacing="trailing").set_timesteps(4)
        assert t.timesteps.tolist() == [999.0, 749.0, 499.0, 249.0] and len(t.sigmas) == 5 and t.sigmas[-1] == 0.0
        train = ((1 - t.alphas_cumprod.astype(np.float64)) / t.alphas_cumprod.astype(np.float64)) ** 0.5
        assert np.array_equal(t.sigmas[:4], train[[999, 749, 499, 249]].astype(np.float32))
        assert cls(timestep_spacing="trailing").set_timesteps(1000).timesteps.tolist() == [float(v) for v in range(999, -1, -1)]


@pytest.mark.parametrize("n", [1, 4, 10, 50, 200])
def test_leading_tables_are_todays(n):
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerAncestralTables, EulerTables, PNDMTables
    for cls, args in ((PNDMTables, ()), (EulerTables, ()), (EulerAncestralTables, ()), (DPMSolverTables, (2,)), (DPMSolverTables, (1, 1000, "sde-dpmsolver++"))):
        if cls is PNDMTables and n < 2:
            continue
        old = cls(*args).set_timesteps(n)
        for kw in (dict(timestep_spacing="leading"), dict(prediction_type="v_prediction"), dict(prediction_type="epsilon", timestep_spacing="leading")):
            new = cls(*args, **kw).set_timesteps(n)
            assert new.kind == old.kind and new.init_noise_sigma == old.init_noise_sigma
            assert torch.equal(torch.as_tensor(new.timesteps), torch.as_tensor(old.timesteps))
            assert torch.equal(torch.tensor(new.table()), torch.tensor(old.table()))
            assert new.prediction_type == kw.get("prediction_type", "epsilon") and old.prediction_type == "epsilon"


def test_bad_keywords_raise():
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerAncestralTables, EulerTables, PNDMTables, engine_prediction
    with pytest.raises(ValueError):
        PNDMTables(timestep_spacing="trailing")
    for cls in (PNDMTables, EulerTables, EulerAncestralTables, DPMSolverTables):
        with pytest.raises(ValueError):
            cls(prediction_type="sample")
        with pytest.raises(ValueError):
            cls(timestep_spacing="linspace")
    s = EulerTables()
    s.prediction_type = "x0"                                  # assigned later: caught when a sampling call reads it
    with pytest.raises(ValueError):
        engine_prediction(s, 5.0)
    with pytest.raises(ValueError):
        engine_prediction(EulerTables(), 5.0, 1.5)


def test_engine_prediction_rule():
    """phi: the call's if > 0, else the pipeline's; only under CFG (guidance_scale > 1, xl.py:903)."""
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerTables, engine_prediction
    assert engine_prediction(EulerTables(), 5.0) == ("epsilon", 0.0)
    assert engine_prediction(EulerTables(), 5.0, 0.7, 0.3) == ("epsilon", 0.7)
    assert engine_prediction(EulerTables(), 5.0, 0.0, 0.3) == ("epsilon", 0.3)
    assert engine_prediction(EulerTables(), 1.0, 0.7, 0.3) == ("epsilon", 0.0)
    assert engine_prediction(DPMSolverTables(prediction_type="v_prediction"), 1.0, 0.7) == ("v_prediction", 0.0)


# ------------------------------------------------------------------------------------------------ command line, checkpoint
def _args(*argv):
    from rich_text_to_image_amd import sample
    return sample.build_parser().parse_args(list(argv))


def test_cli_flags_reach_the_scheduler():
    from rich_text_to_image_amd import sample
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerAncestralTables, EulerTables, PNDMTables
    assert sample.make_scheduler(_args()) is None
    s = sample.make_scheduler(_args("--model", "SDXL", "--prediction_type", "v_prediction", "--timestep_spacing", "trailing"))
    assert type(s) is EulerTables and (s.prediction_type, s.timestep_spacing) == ("v_prediction", "trailing")
    s = sample.make_scheduler(_args("--prediction_type", "v_prediction"))
    assert type(s) is PNDMTables and s.prediction_type == "v_prediction"
    s = sample.make_scheduler(_args("--scheduler", "sde-dpmsolver++", "--timestep_spacing", "trailing", "--solver_order", "1"))
    assert type(s) is DPMSolverTables and (s.kind, s.timestep_spacing, s.prediction_type) == (5, "trailing", "epsilon")
    s = sample.make_scheduler(_args("--model", "AnimeXL", "--scheduler", "euler-ancestral", "--prediction_type", "v_prediction"))
    assert type(s) is EulerAncestralTables and s.prediction_type == "v_prediction"
    assert _args("--guidance_rescale", "0.7").guidance_rescale == 0.7 and _args().guidance_rescale is None


def test_cli_refuses_before_any_rank_starts(tmp_path):
    """main() validates with make_scheduler() before it launches or loads anything."""
    from rich_text_to_image_amd import sample
    for argv in (["--timestep_spacing", "trailing"],                                # PNDM (the SD default) has no trailing list
                 ["--guidance_rescale", "1.5"], ["--guidance_rescale", "-0.1"]):
        with pytest.raises(SystemExit) as e:
            sample.main(argv + ["--rich_text_json", "{}", "--run_dir", str(tmp_path), "--gpus", "2"])
        assert "sample:" in str(e.value), argv
    for argv in (["--prediction_type", "sample"], ["--timestep_spacing", "linspace"]):
        with pytest.raises(SystemExit):
            _args(*argv)


def test_apply_scheduler_keeps_the_checkpoints_prediction_type():
    import types
    from rich_text_to_image_amd import sample
    from rich_text_to_image_amd.schedulers import EulerTables
    model = types.SimpleNamespace(scheduler=EulerTables(prediction_type="v_prediction"))
    sample.apply_scheduler(model, _args("--model", "SDXL", "--scheduler", "dpmsolver++"))
    assert model.scheduler.kind == 3 and model.scheduler.prediction_type == "v_prediction"
    sample.apply_scheduler(model, _args("--model", "SDXL", "--scheduler", "dpmsolver++", "--prediction_type", "epsilon"))
    assert model.scheduler.prediction_type == "epsilon"


@pytest.mark.parametrize("model_type", ["SD", "SDXL"])
def test_generate_carries_guidance_rescale_into_both_passes(monkeypatch, model_type):
    """generate() hands the request's guidance_rescale to both sampling calls: as their keyword, and - the SDXL rich pass, whose keyword
    raises - as the pipeline attribute for the duration of that call only."""
    import types
    from rich_text_to_image_amd import sample
    m1 = torch.ones(1, 4, 2, 2)
    monkeypatch.setattr(sample, "parse_json", lambda *a, **k: ("base", [], [], [], [], [], [], [], False))
    monkeypatch.setattr(sample, "get_region_diffusion_input", lambda *a, **k: (["region", "base"], [[1], [2]], ["base"]))
    monkeypatch.setattr(sample, "get_attention_control_input", lambda *a, **k: {})
    monkeypatch.setattr(sample, "get_gradient_guidance_input", lambda *a, **k: ({}, [[1], [2]]))
    monkeypatch.setattr(sample, "get_token_maps", lambda *a, **k: [m1.clone(), m1.clone()])
    calls = []

    def record(name):
        def f(*a, **k):
            calls.append((name, k.get("run_rich_text"), k.get("guidance_rescale"), model.guidance_rescale))
            return "img"
        return f

    model = types.SimpleNamespace(guidance_rescale=0.25, device="cpu", max_prompt_chunks=1, attention_maps=None, selfattn_maps={}, crossattn_maps={},
                                  n_maps={}, register_tokenmap_hooks=lambda: None, remove_tokenmap_hooks=lambda: None,
                                  produce_attn_maps=record("produce_attn_maps"), prompt_to_img=record("prompt_to_img"), sample=record("sample"))
    param = {"text_input": {}, "height": 16, "width": 16, "guidance_weight": 5.0, "steps": 2, "noise_index": 1, "negative_prompt": ""}
    sample.generate(model, dict(param, guidance_rescale=0.7), model_type)
    if model_type == "SD":
        assert calls == [("produce_attn_maps", None, 0.7, 0.25), ("prompt_to_img", None, 0.7, 0.25)]
    else:
        assert calls == [("sample", False, 0.7, 0.25), ("sample", True, None, 0.7)]
    assert model.guidance_rescale == 0.25
    del calls[:]
    sample.generate(model, param, model_type)                                    # no key: the calls as they always were
    assert [c[2:] for c in calls] == [(None, 0.25), (None, 0.25)]


def test_scheduler_config_sets_the_default(tmp_path):
    from rich_text_to_image_amd.checkpoint import scheduler_prediction_type
    assert scheduler_prediction_type(str(tmp_path)) is None                      # no file: epsilon
    (tmp_path / "scheduler").mkdir()
    f = tmp_path / "scheduler" / "scheduler_config.json"
    f.write_text(json.dumps({"_class_name": "EulerDiscreteScheduler", "beta_schedule": "linear", "timestep_spacing": "trailing"}))
    assert scheduler_prediction_type(str(tmp_path)) is None                      # no key; every other key is ignored
    f.write_text(json.dumps({"_class_name": "DDIMScheduler", "prediction_type": "v_prediction", "rescale_betas_zero_snr": True}))
    assert scheduler_prediction_type(str(tmp_path)) == "v_prediction"
    f.write_text(json.dumps({"prediction_type": "epsilon"}))
    assert scheduler_prediction_type(str(tmp_path)) == "epsilon"
    f.write_text(json.dumps({"prediction_type": "sample"}))
    with pytest.raises(ValueError):
        scheduler_prediction_type(str(tmp_path))
