"""Perturbed-attention guidance on the GPU (csrc/pag.hip, rt_set_pag_layers / rt_set_pag_scales / rt_unet_forward_perturbed): the identity
attention bit for bit with its memory contract, the fold against fp64 at its derived bar, the forward - every stream, the twins far from
their partners, the non-twin streams bit for bit the forward without twins, layer selection by trace bits - and the steps against
tests/pag_ref.py, the split step, graph capture of two steps, off-is-off against digests recorded on the commit before PAG existed, the
refusals and the facade."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import controlnet_ref as CR  # noqa: E402
import pag_ref as R  # noqa: E402
from freeu_ref import FORWARD_BAR, forward_case, oracle_streams, rel_l2  # noqa: E402
from memguard import damage, guarded, intact, poisoned  # noqa: E402
from oracle.unet import OracleUNet  # noqa: E402

DEV = "cuda:0"
STEP_BAR = 3e-2                  # latent UPDATE of one step against the composition of oracle forwards (tests/test_nonsquare_gpu.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pag_off_bits.json")
SIGMAS = (0.0, 2.0, 0.0, 3.0)    # prompt slots [negative, region 0, region 1, base] of rich_case(): region 1 has no twin


# ---------------------------------------------------------------------------------------------------------------- the identity op
ID_SHAPES = [(1, 1, 8, 32), (3, 2, 24, 64), (2, 4, 32, 32), (2, 5, 72, 96), (2, 8, 64, 160), (2, 20, 1000, 64), (2, 20, 1024, 64)]


def _identity(vt, B, H, N, DP, entries, ldvt=None, ldo=None, guard=False):
    """vt: CPU bf16 [H DP, B N].  Returns (O on the CPU [B N, H DP], O's pre-fill on the CPU, (big, window))."""
    from rich_text_to_image_amd.engine import identity_attention
    HD = H * DP
    ldvt, ldo = ldvt or B * N, ldo or HD
    if guard:
        big, ow = guarded((B * N, HD), torch.bfloat16, ldo, fill="bytes", device=DEV)
        vw = poisoned(vt.to(DEV), ldvt)
    else:
        big = None
        ow = torch.full((B * N, ldo), -7.0, dtype=torch.bfloat16, device=DEV)[:, :HD]
        vbuf = torch.full((HD, ldvt), float("nan"), dtype=torch.bfloat16, device=DEV)
        vbuf[:, :B * N] = vt.to(DEV)
        vw = vbuf[:, :B * N]
    before = ow.cpu().clone()
    identity_attention(vw, ow, entries, H, N, DP)
    return ow.cpu(), before, (big, ow)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("B,H,N,DP", ID_SHAPES, ids=[f"B{b}-H{h}-N{n}-DP{d}" for b, h, n, d in ID_SHAPES])
def test_identity_attention_is_the_transpose_bit_for_bit(B, H, N, DP):
    """O = V^T transposed for the named entries, wider leading dimensions, a guarded O window and poisoned V^T padding; a middle entry is
    skipped and keeps its bytes; one entry launched alone equals that entry of the launch of several; a second launch repeats the bits."""
    g = torch.Generator().manual_seed(B * 1000 + N + DP)
    vt = torch.randn(H * DP, B * N, generator=g).bfloat16()
    entries = [b for b in range(B) if not (B >= 3 and b == 1)]
    got, before, (big, ow) = _identity(vt, B, H, N, DP, entries, ldvt=B * N + 8, ldo=H * DP + 16, guard=True)
    assert intact(big, ow), damage(big, ow)
    want = vt.t().contiguous()
    for b in range(B):
        rows = slice(b * N, (b + 1) * N)
        if b in entries:
            assert torch.equal(_bits(got[rows]), _bits(want[rows])), b
        else:
            assert torch.equal(_bits(got[rows]), _bits(before[rows])), b
    again, _, _ = _identity(vt, B, H, N, DP, entries, ldvt=B * N + 8, ldo=H * DP + 16, guard=True)
    assert torch.equal(_bits(again), _bits(got))
    last = B - 1
    one, pre, _ = _identity(vt, B, H, N, DP, [last], ldvt=B * N + 24, ldo=H * DP + 8)
    assert torch.equal(_bits(one[last * N:]), _bits(got[last * N:]))
    assert torch.equal(_bits(one[:last * N]), _bits(pre[:last * N]))
    print(f"identity attention B {B} H {H} N {N} DP {DP}: {len(entries)} of {B} entries, bit-exact")


def test_identity_attention_refuses_what_it_cannot_do():
    from rich_text_to_image_amd.engine import RtError
    B, H, N, DP = 3, 2, 24, 64
    vt = torch.randn(H * DP, B * N).bfloat16()
    bad = [dict(N=20), dict(DP=48), dict(ldvt=B * N + 4), dict(ldo=H * DP + 4), dict(entries=[0, 0]), dict(entries=[0, 3]), dict(entries=[-1])]
    for kw in bad:
        a = dict(B=B, H=H, N=N, DP=DP, entries=[0, 2], ldvt=None, ldo=None)
        a.update(kw)
        n, dp = a["N"], a["DP"]
        v = torch.randn(H * dp, B * n).bfloat16() if (n, dp) != (N, DP) else vt
        with pytest.raises(RtError) as e:
            got, before, _ = _identity(v, B, H, n, dp, a["entries"], ldvt=a["ldvt"], ldo=a["ldo"])
        assert e.value.code == -1, kw
    # nothing is written by a refused call
    from rich_text_to_image_amd.engine import identity_attention
    o = torch.full((B * N, H * DP), -7.0, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RtError):
        identity_attention(vt.to(DEV), o, [0, 0], H, N, DP)
    assert bool((o == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------- the fold op
@pytest.mark.parametrize("h,w", [(8, 8), (16, 24), (128, 128)], ids=["8x8", "16x24", "128x128"])
def test_fold_matches_fp64(h, w):
    """Three of nine streams folded: within 2^-23 (|rho| |t - p| + |ref|) of fp64; unnamed streams and the twins keep their bytes; the
    input itself (a dropped fold) lies outside the bar on more than 90 % of the elements."""
    from rich_text_to_image_amd.engine import pag_fold
    g = torch.Generator().manual_seed(h * 100 + w)
    eps = torch.randn(9, h * w, 4, generator=g)
    s, tw, rho = [1, 3, 4], [6, 7, 8], [3.0 / 5.0, 0.4, -0.25]
    got = pag_fold(eps.to(DEV).clone(), h, w, s, tw, rho).cpu()
    worst = 0.0
    for si, ti, r in zip(s, tw, rho):
        ref, bar = R.fold_ref(eps[si], eps[ti], r), R.fold_bar(eps[si], eps[ti], r)
        err = (got[si].double() - ref).abs()
        worst = max(worst, float((err / bar.clamp_min(1e-300)).max()))
        assert bool((err <= bar).all()), (si, worst)
        assert float(((eps[si].double() - ref).abs() > bar).double().mean()) > 0.9
    for b in range(9):
        if b not in s:
            assert torch.equal(got[b].view(torch.int32), eps[b].view(torch.int32)), b
    print(f"pag fold {h}x{w}: worst |got - ref| / bar = {worst:.3f}")
    again = pag_fold(eps.to(DEV).clone(), h, w, s, tw, rho).cpu()
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))


def test_fold_refuses_what_it_cannot_do():
    from rich_text_to_image_amd.engine import RtError, pag_fold
    eps = torch.randn(4, 64, 4, device=DEV)
    keep = eps.clone()
    for s, tw, rho in (([1], [1], [0.5]), ([1, 1], [2, 3], [0.5, 0.5]), ([1, 2], [3, 3], [0.5, 0.5]), ([1, 2], [2, 3], [0.5, 0.5]), ([4], [0], [0.5]),
                       ([1], [-1], [0.5]), ([1], [2], [float("nan")])):
        with pytest.raises(RtError) as e:
            pag_fold(eps, 8, 8, s, tw, rho)
        assert e.value.code == -1, (s, tw, rho)
        assert torch.equal(eps, keep)


# ---------------------------------------------------------------------------------------------------------------- engines
def _engine(cfg, h, w, sd, **kw):
    from rich_text_to_image_amd.engine import Engine
    e = Engine(cfg, h, w, device=0, **kw)
    e.load_state_dict(sd)
    assert e.weights_missing()[0] == 0
    return e


def _set_prompts(eng, c):
    if c["xl"]:
        eng.set_prompts(c["emb"].to(DEV), c["pooled"].to(DEV), c["tid"])
    else:
        eng.set_prompts(c["emb"].to(DEV))
    eng.set_fontsize(c["wp"], c["fs"])


FWD = dict(prompt=[0, 2, 2, 1, 2, 1], fontsize=[0, 1, 0, 0, 1, 0], qk_src=[0, 1, 2, 2, 4, 2], res_src=[-1, -1, -1, 2, -1, 2], perturb=[0, 0, 0, 0, 1, 1])


def _forward(eng, c, twins=True, trace=None):
    """[uncond, base + font size, text_ref, injected region, twin of base, twin of the injected region] (or the first four alone)."""
    n = 6 if twins else 4
    x = torch.cat([c["lat"], c["lat"], c["lat_ref"], c["lat"], c["lat"], c["lat"]][:n]).to(DEV)
    out = eng.unet_forward(x, c["t"], FWD["prompt"][:n], fontsize=FWD["fontsize"][:n], qk_src=FWD["qk_src"][:n], res_src=FWD["res_src"][:n],
                           perturb=FWD["perturb"][:n] if twins else None, trace=trace)
    return (out[0].cpu(), out[1].cpu()) if trace else out.cpu()


def _oracle_twins(c, applied):
    """The twins of base (+ font size) and of the injected region on PagOracleUNet."""
    from oracle.unet import INJECT_RESNET
    o, op = OracleUNet(c["cfg"], c["sd"]), R.PagOracleUNet(c["cfg"], c["sd"], applied)

    def added(k):
        return {"text_embeds": c["pooled"][k:k + 1], "time_ids": c["tid"]} if c["xl"] else None
    emb, t = c["emb"], c["t"]
    with torch.no_grad():
        p_base = op.forward(c["lat"], t, emb[2:3], added(2), ctl={"fontsize": {"word_pos": c["wp"], "font_size": c["fs"]}})
        cap = {}
        o.forward(c["lat_ref"], t, emb[2:3], added(2), ctl={"capture": cap})
        inj = {k: v for k, v in cap.items() if k.endswith("attn1") or k == INJECT_RESNET}
        p_reg = op.forward(c["lat"], t, emb[1:2], added(1), ctl={"inject": inj})
    return [p_base[0], p_reg[0]]


@pytest.mark.parametrize("which", ["xl", "sd"])
def test_forward_with_twins_matches_the_oracle(which):
    """All attn1 modules applied: every stream within FORWARD_BAR of its oracle, the twins at least 10 x FORWARD_BAR from their partners,
    the four non-twin streams bit for bit the forward without twins.  With layers = mid only: the twin's trace at the last traceable
    module before mid_block's attention - mid_block.resnets.0, behind every down block and the first resnet of the mid block itself -
    equals its partner's bits, at mid_block.attentions.0 it differs."""
    from rich_text_to_image_amd.pag import resolve_layers
    c = forward_case(which)
    eng = _engine(c["cfg"], c["h"], c["w"], c["sd"])
    try:
        _set_prompts(eng, c)
        plain = _forward(eng, c, twins=False)
        every = resolve_layers(("down", "mid", "up"), eng.attn_modules())
        assert every == R.all_attn1(c["cfg"])
        eng.set_pag_layers(every)
        assert torch.equal(_forward(eng, c, twins=False), plain)           # applied layers without a perturbed stream change nothing
        got = _forward(eng, c)
        assert torch.equal(got[:4], plain), "a non-twin stream's bits depend on the twins"
        refs = oracle_streams(OracleUNet(c["cfg"], c["sd"]), c) + _oracle_twins(c, every)
        errs = [rel_l2(got[i], refs[i]) for i in range(6)]
        far = [rel_l2(got[4], got[1]), rel_l2(got[5], got[3])]
        print(f"forward with twins ({which}): rel-L2 per stream {['%.3e' % e for e in errs]}; twins from their partners {['%.3f' % f for f in far]}")
        assert max(errs) <= FORWARD_BAR, errs
        assert min(far) >= 10 * FORWARD_BAR, far
        # layer selection, by bits
        mid = resolve_layers(("mid",), eng.attn_modules())
        assert mid and all(n.startswith("mid_block.") for n in mid)
        eng.set_pag_layers(mid)
        names = [n for n, _, _ in eng.trace_modules()]
        before_mid = names[names.index("mid_block.resnets.0")]
        _, tr = _forward(eng, c, trace=before_mid)
        assert torch.equal(tr[4], tr[1]) and torch.equal(tr[5], tr[3])
        _, tr = _forward(eng, c, trace="mid_block.attentions.0")
        assert not torch.equal(tr[4], tr[1]) and not torch.equal(tr[5], tr[3])
        eng.set_pag_layers([])
        assert torch.equal(_forward(eng, c, twins=False), plain)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- steps
def _rich_setup(eng, c, sigmas=SIGMAS, layers=None):
    from rich_text_to_image_amd.pag import resolve_layers
    eng.set_prompts(c["emb"].to(DEV), c["pooled"].to(DEV), c["tid"])
    eng.set_masks(c["masks"].to(DEV))
    eng.set_fontsize(torch.tensor([3, 5]), torch.tensor([4.0, -2.0]))
    if sigmas is not None:
        eng.set_pag_layers(resolve_layers(layers or ("down", "mid", "up"), eng.attn_modules()))
        eng.set_pag_scales(sigmas)


def _rich_reset(eng, c):
    eng.set_schedule(0, c["sched"].timesteps.tolist(), c["sched"].sigmas.tolist(), c["steps"])
    eng.set_latents(c["lat"].to(DEV))


@pytest.fixture(scope="module")
def rich():
    c = CR.rich_case()
    eng = _engine(c["cfg"], c["hw"], c["hw"], c["sd"], max_streams=12)
    _rich_setup(eng, c)
    yield c, eng
    eng.close()


def _added_fn(c):
    def added_fn(k):
        k = k if k >= 0 else c["pooled"].shape[0] + k
        return {"text_embeds": c["pooled"][k:k + 1], "time_ids": c["tid"]}
    return added_fn


def test_region_step_matches_the_composition_of_oracle_forwards(rich):
    """The injected first region_step on tiny XL (Euler), R = 3, sigma = (base 3.0, region 0 2.0, region 1 0): 9 streams; both latent
    streams after the scheduler step against the three-term guidance of oracle forwards, on the latent UPDATE, at guidance scale
    pag_ref.STEP_GS; the step without PAG is far away.  (Measured on an MI355X: 2.41e-2 / 2.88e-2 main / reference stream at g = 3; at
    rich_case's own g = 5 - before STEP_GS was introduced for the CPU discrimination test - 3.24e-2 / 3.55e-2, over the bar: sigma (T - P)
    is a difference of two bf16 forwards, each 8e-3 from its oracle, that share less rounding than T and u do.)"""
    c, eng = rich
    hw, R_ = c["hw"], c["masks"].shape[0]
    _rich_reset(eng, c)
    info = eng.region_step_part(0, R.STEP_GS, c["isa"], 0.0, True, 0, 1)[2]
    assert info[0] == 9, info
    _rich_reset(eng, c)
    eng.region_step(0, R.STEP_GS, c["isa"], 0.0, xl=True)
    got, got_ref = (t.cpu() for t in eng.read_latents(hw, hw, with_ref=True))
    sched, lat0, gs = c["sched"], c["lat"], R.STEP_GS
    t = sched.timesteps[0]
    assert float(t) > (1 - c["isa"]) * 1000
    every = R.all_attn1(c["cfg"])
    o, op = OracleUNet(c["cfg"], c["sd"]), R.PagOracleUNet(c["cfg"], c["sd"], every)
    lat_in = sched.scale_model_input(lat0, t)
    tfd = {"word_pos": torch.tensor([3, 5]), "font_size": torch.tensor([4.0, -2.0])}
    masks = [c["masks"][r:r + 1] for r in range(R_)]

    def compose(sig):
        e, er = R.rich_step_pag(o, op, lat_in, lat_in.clone(), t, c["emb"], _added_fn(c), masks, tfd, True, sig, gs)
        out = sched.step(torch.cat([e, er]).float(), t, torch.cat([lat0, lat0]))["prev_sample"]
        return torch.chunk(out, 2, dim=0)
    ref, ref_ref = compose(SIGMAS)
    off, off_ref = compose((0.0,) * 4)
    r, rr = rel_l2(got - lat0, ref - lat0), rel_l2(got_ref - lat0, ref_ref - lat0)
    d, dr = rel_l2(off - lat0, ref - lat0), rel_l2(off_ref - lat0, ref_ref - lat0)
    print(f"region_step with PAG: latent UPDATE rel-L2 {r:.3e} (reference stream {rr:.3e}); the step without PAG is {d:.3e} / {dr:.3e} away")
    assert r <= STEP_BAR and rr <= STEP_BAR
    assert d > 3 * STEP_BAR and dr > 3 * STEP_BAR


@pytest.mark.parametrize("vpred", [False, True], ids=["epsilon", "v"])
def test_plain_step_matches_the_composition_of_oracle_forwards(vpred):
    """plain_step (streams [uncond, text, twin of text]) with sigma 3.0 on the text slot; once with v-prediction (the fold composes with
    the conversion: everything is linear)."""
    c = CR.rich_case()
    hw = c["hw"]
    eng = _engine(c["cfg"], hw, hw, c["sd"])
    try:
        emb, pooled = c["emb"][[0, 3]], c["pooled"][[0, 3]]
        eng.set_prompts(emb.to(DEV), pooled.to(DEV), c["tid"])
        every = R.all_attn1(c["cfg"])
        eng.set_pag_layers(every)
        eng.set_pag_scales([0.0, 3.0])
        eng.set_prediction(1 if vpred else 0, 0.0)
        _rich_reset(eng, c)
        eng.plain_step(0, R.STEP_GS)
        got = eng.read_latents(hw, hw).cpu()
        eng.set_pag_scales([0.0, 0.0])
        _rich_reset(eng, c)
        eng.plain_step(0, R.STEP_GS)
        got_off = eng.read_latents(hw, hw).cpu()
    finally:
        eng.close()
    sched, lat0, gs = c["sched"], c["lat"], R.STEP_GS
    t = sched.timesteps[0]
    sigma = float(sched.sigmas[0])
    x = sched.scale_model_input(lat0, t)
    o, op = OracleUNet(c["cfg"], c["sd"]), R.PagOracleUNet(c["cfg"], c["sd"], every)

    def added(k):
        return {"text_embeds": pooled[k:k + 1], "time_ids": c["tid"]}
    with torch.no_grad():
        eu, et, ep = o.forward(x, t, emb[:1], added(0)), o.forward(x, t, emb[1:], added(1)), op.forward(x, t, emb[1:], added(1))

    def compose(sig):
        m = R.guidance_ref(eu, [et], [ep], [torch.ones_like(et)], [sig], gs)
        if vpred:                                                       # include/rtdiff.h, rt_set_prediction: sigma space
            m = m / (sigma ** 2 + 1) ** 0.5 + lat0.double() * sigma / (sigma ** 2 + 1)
        return sched.step(m.float(), t, lat0)["prev_sample"]
    ref, off = compose(3.0), compose(0.0)
    r, d, ro = rel_l2(got - lat0, ref - lat0), rel_l2(off - lat0, ref - lat0), rel_l2(got_off - lat0, off - lat0)
    print(f"plain_step with PAG ({'v' if vpred else 'epsilon'}): latent UPDATE rel-L2 {r:.3e} (PAG off: {ro:.3e}); the step without PAG is {d:.3e} away")
    assert r <= STEP_BAR and ro <= STEP_BAR
    # a property of the two oracle compositions alone: a result within STEP_BAR of the PAG composition is then closer to it than to the
    # composition without PAG (under v-prediction the latents' own share of the update shrinks the relative distance: 0.069 against 0.49)
    assert d > 2 * STEP_BAR


# tiny SD (PNDM, DPM-Solver++): two steps, so that the multistep history of both solvers carries folded predictions
def _sd_case():
    from oracle.unet import TINY_SD_CONFIG, random_state_dict
    cfg = TINY_SD_CONFIG
    g = torch.Generator().manual_seed(31)
    hw, R_ = 32, 3
    return dict(cfg=cfg, sd=random_state_dict(cfg, seed=12), hw=hw, masks=torch.softmax(torch.randn(R_, 1, hw, hw, generator=g) * 2, 0).repeat(1, 4, 1, 1),
                emb=torch.randn(R_ + 1, 77, cfg["cross_attention_dim"], generator=g), lat=torch.randn(1, 4, hw, hw, generator=g), n=5, isa=0.5,
                tfd={"word_pos": torch.tensor([3, 5]), "font_size": torch.tensor([4.0, -2.0])})


def _sd_schedule(eng, solver, n):
    """Sets the engine's schedule and returns the oracle scheduler of the same solver."""
    if solver == "pndm":
        from oracle.schedulers import OraclePNDM
        from rich_text_to_image_amd.schedulers import PNDMTables
        t = PNDMTables().set_timesteps(n)
        eng.set_schedule(1, t.timesteps.tolist(), t.table(), n)
        o = OraclePNDM()
    else:
        from dpm_solver_ref import RefDPMSolver, dpm_timesteps, scaled_linear_alphas_cumprod
        eng.set_schedule(3, [float(t) for t in dpm_timesteps(n)], scaled_linear_alphas_cumprod().tolist(), n)
        o = RefDPMSolver(2)
    o.set_timesteps(n)
    return o


@pytest.mark.parametrize("solver", ["pndm", "dpmpp2"])
def test_sd_steps_match_the_composition_of_oracle_forwards(solver):
    """Tiny SD, R = 3, injection on, sigma = (base 3.0, region 0 2.0, region 1 0), all layers applied, guidance scale pag_ref.STEP_GS: the
    first TWO region steps and the first two plain steps under PNDM / DPM-Solver++ (order 2).  Step 0 against the composition of oracle
    forwards from the start latents; step 1 against the composition evaluated at the engine's own latents after step 0, stepped by the
    oracle scheduler that holds the ORACLE's step-0 prediction as its history - so the second step pins that the solver's history carries
    the folded prediction.  Latent UPDATE (from the start latents) <= STEP_BAR, latents_reference too."""
    c = _sd_case()
    hw, gs, lat0 = c["hw"], R.STEP_GS, c["lat"]
    every = R.all_attn1(c["cfg"])
    o, op = OracleUNet(c["cfg"], c["sd"]), R.PagOracleUNet(c["cfg"], c["sd"], every)
    masks = [c["masks"][r:r + 1] for r in range(3)]
    eng = _engine(c["cfg"], hw, hw, c["sd"], max_streams=12)
    try:
        # ---- the rich pass
        eng.set_prompts(c["emb"].to(DEV))
        eng.set_masks(c["masks"].to(DEV))
        eng.set_fontsize(c["tfd"]["word_pos"], c["tfd"]["font_size"])
        eng.set_pag_layers(every)
        eng.set_pag_scales(SIGMAS)
        sched = _sd_schedule(eng, solver, c["n"])
        eng.set_latents(lat0.to(DEV))
        x, xr = lat0, lat0.clone()
        for i in range(2):
            t = sched.timesteps[i]
            feat = bool(t > (1 - c["isa"]) * 1000)
            assert feat
            e, er = R.rich_step_pag(o, op, x, xr, t, c["emb"], lambda k: None, masks, c["tfd"], feat, SIGMAS, gs)
            ref, ref_ref = torch.chunk(sched.step(torch.cat([e, er]).float(), t, torch.cat([x, xr]))["prev_sample"], 2, dim=0)
            eng.region_step(i, gs, c["isa"], 0.0, xl=False)
            got, got_ref = (v.cpu() for v in eng.read_latents(hw, hw, with_ref=True))
            r, rr = rel_l2(got - lat0, ref - lat0), rel_l2(got_ref - lat0, ref_ref - lat0)
            print(f"tiny SD {solver} region step {i} with PAG: latent UPDATE rel-L2 {r:.3e} (reference stream {rr:.3e})")
            assert r <= STEP_BAR and rr <= STEP_BAR, (i, r, rr)
            x, xr = got, got_ref
        # ---- the plain pass
        emb = c["emb"][[0, 3]]
        eng.set_prompts(emb.to(DEV))
        eng.set_fontsize(None, None)
        eng.set_pag_scales([0.0, 3.0])
        sched = _sd_schedule(eng, solver, c["n"])
        eng.set_latents(lat0.to(DEV))
        x = lat0
        for i in range(2):
            t = sched.timesteps[i]
            with torch.no_grad():
                eu, et, ep = o.forward(x, t, emb[:1]), o.forward(x, t, emb[1:]), op.forward(x, t, emb[1:])
            ref = sched.step(R.guidance_ref(eu, [et], [ep], [torch.ones_like(et)], [3.0], gs).float(), t, x)["prev_sample"]
            eng.plain_step(i, gs)
            got = eng.read_latents(hw, hw).cpu()
            r = rel_l2(got - lat0, ref - lat0)
            print(f"tiny SD {solver} plain step {i} with PAG: latent UPDATE rel-L2 {r:.3e}")
            assert r <= STEP_BAR, (i, r)
            x = got
    finally:
        eng.close()


def test_stream_plan_counts_the_twins(rich):
    """plan_info[0] of rt_region_step_part against pag.expected_streams for R = 3, sigma = (base 3.0, region 0 2.0, region 1 0): injected,
    not injected with the pair stepped, the pair run but not stepped, the pair elided."""
    from rich_text_to_image_amd.pag import expected_streams
    c, eng = rich
    _rich_reset(eng, c)
    n = c["steps"]
    assert n == 3
    #        step, isa, ibg, elide | inject, step_ref, run_ref
    cases = [(0, 0.5, 0.0, False, True, True, True), (0, 0.0, 0.4, False, False, True, True), (2, 0.0, 0.4, False, False, False, True),
             (2, 0.0, 0.4, True, False, False, False)]
    for i, isa, ibg, elide, inject, step_ref, run_ref in cases:
        want = expected_streams(3, SIGMAS, inject, step_ref, run_ref)
        # only the plan is asked for: part 62 of 64 is empty for every stream count here and runs no forward
        first, count, (F, s_tref, inj) = eng.region_step_part(i, c["gs"], isa, ibg, True, 62, 64, elide=elide)
        assert count == 0
        assert (F, inj, s_tref) == (len(want), inject, 3 if run_ref else -1), (i, isa, ibg, elide, F, want)
    _rich_reset(eng, c)


def test_reference_pair_retraces_the_plain_pass(rich):
    """The reference stream of the rich pass fed the plain pass's inputs gives the plain pass's latents bit for bit with PAG on: the pair
    gets u_ref + g (T_ref - u_ref) + sigma_base (T_ref - P_ref)."""
    c, eng = rich
    hw = c["hw"]
    _rich_reset(eng, c)
    eng.region_step(0, c["gs"], c["isa"], 0.0, xl=True)
    _, ref = eng.read_latents(hw, hw, with_ref=True)
    ref = ref.clone()
    plain = _engine(c["cfg"], hw, hw, c["sd"])
    try:
        plain.set_prompts(c["emb"][[0, 3]].to(DEV), c["pooled"][[0, 3]].to(DEV), c["tid"])
        plain.set_pag_layers(R.all_attn1(c["cfg"]))
        plain.set_pag_scales([0.0, SIGMAS[3]])
        _rich_reset(plain, c)
        plain.plain_step(0, c["gs"])
        assert torch.equal(plain.read_latents(hw, hw), ref)
    finally:
        plain.close()


def test_split_step_equals_the_whole_step(rich):
    """rt_region_step_part for both parts of two, then _finish, gives the bits of rt_region_step; likewise the plain step, whose twin
    rides with the text stream's part."""
    c, eng = rich
    hw = c["hw"]
    for i in (0, c["steps"] - 1):
        _rich_reset(eng, c)
        eng.region_step(i, c["gs"], c["isa"], c["ibg"], xl=True)
        whole = [t.clone() for t in eng.read_latents(hw, hw, with_ref=True)]
        _rich_reset(eng, c)
        ranges = [eng.region_step_part(i, c["gs"], c["isa"], c["ibg"], True, part, 2)[:2] for part in (0, 1)]
        assert all(n > 0 for _, n in ranges), ranges
        eng.region_step_finish(i, c["gs"], c["isa"], c["ibg"], True)
        parts = eng.read_latents(hw, hw, with_ref=True)
        assert torch.equal(parts[0], whole[0]) and torch.equal(parts[1], whole[1]), i
    # the plain step: prompts [negative, region 0]; slot 1 has sigma 2.0
    _rich_reset(eng, c)
    eng.plain_step(0, c["gs"])
    whole = eng.read_latents(hw, hw).clone()
    _rich_reset(eng, c)
    assert [eng.plain_step_part(0, part, 2) for part in (0, 1)] == [(0, 1), (1, 2)]
    eng.plain_step_finish(0, c["gs"])
    assert torch.equal(eng.read_latents(hw, hw), whole)


def test_two_pag_steps_are_hipgraph_capturable(rich):
    """As the ControlNet graph test with PAG on, over TWO steps: nothing is allocated and nothing synchronises inside a step (the entry
    lists and ratios travel in the kernel arguments), and the replay gives the eager steps' bits."""
    c, eng = rich
    hw = c["hw"]

    def two_steps():
        eng.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True)
        eng.region_step(1, c["gs"], c["isa"], c["ibg"], xl=True)
    _rich_reset(eng, c)
    two_steps()
    eager = eng.read_latents(hw, hw).clone()
    side = torch.cuda.Stream()
    eng.synchronize()
    eng.set_stream(side.cuda_stream)
    try:
        _rich_reset(eng, c)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            two_steps()
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


def test_pag_launches_are_profiled_under_their_own_class(rich):
    c, eng = rich
    _rich_reset(eng, c)
    eng.profile_enable(True)
    eng.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True)
    eng.synchronize()
    p = eng.profile_read_pag()
    eng.profile_enable(False)
    assert p["launches"] == len(R.all_attn1(c["cfg"])) + 1 and p["total_bytes"] > 0 and p["total_flops"] == 0, p
    _rich_reset(eng, c)


# ---------------------------------------------------------------------------------------------------------------- off is off
def test_off_is_off_against_the_bits_of_the_commit_before():
    """tests/golden/pag_off_bits.json holds the sha256 of the tiny forwards and of one region step, recorded on the GPU by
    controlnet_ref.off_digests on the commit before PAG existed.  This tree reproduces them with no PAG set, with layers set and every
    sigma 0, and after a request was switched off again; no RT_PROF_PAG launch is counted."""
    with open(GOLDEN) as f:
        want = json.load(f)["digests"]
    counted = []

    def profiled(cfg, h, w, sd):
        eng = _engine(cfg, h, w, sd)
        eng.profile_enable(True)
        close = eng.close

        def close_and_count():
            if eng.h:
                counted.append(eng.profile_read_pag()["launches"])
            close()
        eng.close = close_and_count
        return eng

    def zero_scales(eng, c):
        eng.set_pag_layers(R.all_attn1(c["cfg"]))
        eng.set_pag_scales([0.0] * c["emb"].shape[0])

    def on_then_off(eng, c):
        n = c["emb"].shape[0]
        eng.set_pag_layers(R.all_attn1(c["cfg"]))
        eng.set_pag_scales([0.0] + [3.0] * (n - 1))
        eng.set_pag_scales([0.0] * n)
        eng.set_pag_layers([])
    assert CR.off_digests(profiled) == want
    assert CR.off_digests(profiled, zero_scales) == want
    assert CR.off_digests(profiled, on_then_off) == want
    assert counted and all(n == 0 for n in counted), counted


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_engine_usable(rich):
    """Every refusal is RT_E_INVALID before any launch and leaves the state alone: the next step keeps its bits."""
    from rich_text_to_image_amd.engine import RtError
    c, eng = rich
    hw = c["hw"]

    def step():
        _rich_reset(eng, c)
        eng.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True)
        return eng.read_latents(hw, hw).clone()
    before = step()
    every = R.all_attn1(c["cfg"])

    def refused(call, *words):
        with pytest.raises(RtError) as e:
            call()
        assert e.value.code == -1, str(e.value)
        for wd in words:
            assert wd in str(e.value), (wd, str(e.value))
        assert torch.equal(step(), before)
    refused(lambda: eng.set_pag_scales([1.0, 2.0, 0.0, 3.0]), "negative")
    refused(lambda: eng.set_pag_scales([0.0, float("nan"), 0.0, 3.0]), "slot 1")
    refused(lambda: eng.set_pag_scales([0.0, 2.0, float("inf"), 3.0]), "slot 2")
    refused(lambda: eng.set_pag_scales(list(SIGMAS) + [1.0]))
    refused(lambda: eng.set_pag_scales([]))
    refused(lambda: eng.set_pag_layers(["mid_block.attentions.0.transformer_blocks.9.attn1"]), "transformer_blocks.9.attn1")
    refused(lambda: eng.set_pag_layers([every[0][:-1] + "2"]), "attn2")
    refused(lambda: eng.set_pag_layers([]), "empty")
    # the two combinations, before any launch
    _rich_reset(eng, c)
    lat0 = eng.read_latents(hw, hw).clone()
    with pytest.raises(RtError) as e:
        eng.region_step(0, 0.0, c["isa"], c["ibg"], xl=True)
    assert e.value.code == -1 and "guidance_scale" in str(e.value)
    assert torch.equal(eng.read_latents(hw, hw), lat0)
    eng.set_prediction(0, 0.5)
    for call in (lambda: eng.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True), lambda: eng.plain_step(0, c["gs"])):
        with pytest.raises(RtError) as e:
            call()
        assert e.value.code == -1 and "guidance_rescale" in str(e.value)
        assert torch.equal(eng.read_latents(hw, hw), lat0)
    with pytest.raises(RtError) as e:                                        # the split plain step: the rescale is refused by the part call, before its forward
        eng.plain_step_part(0, 1, 2)
    assert e.value.code == -1 and "guidance_rescale" in str(e.value)
    eng.set_prediction(0, 0.0)
    assert torch.equal(step(), before)
    # more streams than the engine was built for: both numbers are named
    small = _engine(c["cfg"], hw, hw, c["sd"], max_streams=7)
    try:
        _rich_setup(small, c)
        _rich_reset(small, c)
        with pytest.raises(RtError) as e:
            small.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True)
        assert e.value.code == -1 and "max_streams 7" in str(e.value) and "8" in str(e.value), str(e.value)
        small.set_pag_scales([0.0] * 4)
        _rich_reset(small, c)
        small.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True)         # still usable
    finally:
        small.close()
    # an empty applied set with a sigma, the other way round
    fresh = _engine(c["cfg"], hw, hw, c["sd"])
    try:
        fresh.set_prompts(c["emb"].to(DEV), c["pooled"].to(DEV), c["tid"])
        with pytest.raises(RtError) as e:
            fresh.set_pag_scales(SIGMAS)
        assert e.value.code == -1 and "empty" in str(e.value)
        x = c["lat"].to(DEV)
        with pytest.raises(RtError):                                         # a perturbed stream without an applied layer
            fresh.unet_forward(torch.cat([x, x]), 500.0, [0, 3], perturb=[0, 1])
        with pytest.raises(RtError):                                         # twins must trail
            fresh.set_pag_layers(every)
            fresh.unet_forward(torch.cat([x, x]), 500.0, [3, 0], perturb=[1, 0])
        assert bool(torch.isfinite(fresh.unet_forward(x, 500.0, [3])).all())
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------- facade
def _facade(which, c):
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    from rich_text_to_image_amd.region_diffusion_sdxl import RegionDiffusionXL
    m = RegionDiffusionXL(device=0, unet_state_dict=c["sd"], config=c["cfg"]) if which == "xl" else RegionDiffusion(0, unet_state_dict=c["sd"], config=c["cfg"])
    m.masks = [c["masks"][r:r + 1] for r in range(c["masks"].shape[0])]
    return m


def test_facade_xl_set_pag_changes_the_image_and_clear_pag_restores_it(monkeypatch):
    c = CR.rich_case()
    hw, n = c["hw"], 3
    tfd = {"word_pos": torch.tensor([3, 5]), "font_size": torch.tensor([4.0, -2.0])}

    def sample(m, rich=True, **kw):
        return m.sample(prompt=None, height=8 * hw, width=8 * hw, num_inference_steps=n, guidance_scale=c["gs"], latents=c["lat"].clone() / c["sched"].init_noise_sigma,
                        prompt_embeds=c["emb"][1:] if rich else c["emb"][-1:], negative_prompt_embeds=c["emb"][:1],
                        pooled_prompt_embeds=c["pooled"][1:] if rich else c["pooled"][-1:], negative_pooled_prompt_embeds=c["pooled"][:1], output_type="latent",
                        run_rich_text=rich, text_format_dict=tfd, inject_selfattn=c["isa"], inject_background=c["ibg"], **kw).images.cpu()
    m = _facade("xl", c)
    never, never_plain = sample(m), sample(m, rich=False)
    m.set_pag(scale=3.0, regions={1: 0.0}, layers=("down", "mid", "up"))
    on = sample(m)
    assert rel_l2(on, never) > 1e-2 and torch.equal(sample(m), on)
    assert rel_l2(sample(m, rich=False), never_plain) > 1e-2
    with pytest.raises(ValueError):
        sample(m, guidance_rescale=0.5, rich=False)
    with pytest.raises(ValueError):                                          # region 2 of a request with two region prompts
        m.set_pag(regions={2: 1.0})
        sample(m)
    m.set_pag(scale=0.0)
    assert torch.equal(sample(m), never)
    m.clear_pag()
    assert torch.equal(sample(m), never) and torch.equal(sample(m, rich=False), never_plain)
    # a --requests line with `pag` does not leak into the next request: sample.generate's set-and-restore around REAL sampling calls on one
    # pipeline, whose engine is reused (and was grown for the twins) - sigma and the applied layers must not survive on it
    from rich_text_to_image_amd import sample as S
    monkeypatch.setattr(S, "_generate", lambda model, param, *a: (sample(model, rich=False), sample(model), {}))
    m2 = _facade("xl", c)
    req = dict(scale=3.0, regions={1: 0.0}, base=None, layers=("down", "mid", "up"))
    plain_on, rich_on, _ = S.generate(m2, {"pag": req})
    assert torch.equal(rich_on, on) and rel_l2(plain_on, never_plain) > 1e-2 and m2.pag is None
    plain_off, rich_off, _ = S.generate(m2, {"pag": None})
    assert torch.equal(rich_off, never) and torch.equal(plain_off, never_plain)
    plain_on2, rich_on2, _ = S.generate(m2, {"pag": req})
    assert torch.equal(rich_on2, on) and torch.equal(plain_on2, plain_on)


def test_facade_sd_set_pag_changes_the_image_and_clear_pag_restores_it():
    from oracle.unet import TINY_SD_CONFIG, random_state_dict
    cfg = TINY_SD_CONFIG
    g = torch.Generator().manual_seed(31)
    hw, R_, n = 32, 3, 4
    c = dict(cfg=cfg, sd=random_state_dict(cfg, seed=12), masks=torch.softmax(torch.randn(R_, 1, hw, hw, generator=g) * 2, 0).repeat(1, 4, 1, 1))
    emb = torch.randn(R_ + 1, 77, cfg["cross_attention_dim"], generator=g)
    lat = torch.randn(1, 4, hw, hw, generator=g)

    def rich(m):
        return m.produce_latents(emb, height=8 * hw, width=8 * hw, num_inference_steps=n, guidance_scale=7.5, latents=lat.clone(),
                                 inject_selfattn=0.5, inject_background=0.4).cpu()

    def plain(m):
        return m.plain_latents(emb[[0, R_]], 8 * hw, 8 * hw, n, 7.5, lat.clone()).cpu()
    m = _facade("sd", c)
    never_r, never_p = rich(m), plain(m)
    m.set_pag(scale=2.0, base=3.0, layers=("down", "mid", "up"))
    on_r, on_p = rich(m), plain(m)
    assert rel_l2(on_r, never_r) > 1e-2 and rel_l2(on_p, never_p) > 1e-2
    assert torch.equal(rich(m), on_r) and torch.equal(plain(m), on_p)
    m.clear_pag()
    assert torch.equal(rich(m), never_r) and torch.equal(plain(m), never_p)
