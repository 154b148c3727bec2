"""Image prompts on the GPU (csrc/ipattn.hip, rt_set_image_prompts / rt_op_ip_attention): the op against the fp64 restatement of
tests/ip_adapter_ref.py at its derived bar, batch invariance, the memory contract, off-is-off, the forward and the steps against the
oracle with the image term plugged in, the split step, graph capture, the refusals and the facade."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import ip_adapter_ref as R  # noqa: E402
from freeu_ref import FORWARD_BAR, forward_case, oracle_streams, rel_l2  # noqa: E402
from memguard import damage, guarded, intact, poisoned  # noqa: E402
from oracle.region_loop import rich_step_forwards  # noqa: E402
from oracle.schedulers import OracleEuler  # noqa: E402
from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, OracleUNet, random_state_dict  # noqa: E402

DEV = "cuda:0"
STEP_BAR = 3e-2                  # latent UPDATE of one step against the composition of oracle forwards (tests/test_nonsquare_gpu.py)


# ---------------------------------------------------------------------------------------------------------------- the op
def _launch(Q, K, V, O, slots, counts, scales, ldq=None, ldo=None, ldvt=None, guard=False):
    """The op on CPU tensors Q, O [B, N, H, DP], K, V [nslot, 16, H, DP] in the engine's layouts: Q / O rows of H DP columns with leading
    dimensions ldq / ldo, K rows (slot, key), V^T [H DP, 16 nslot] with leading dimension ldvt.  guard: every operand in a guarded /
    poisoned window (tests/memguard.py); returns (O after, the guard check of O)."""
    from rich_text_to_image_amd.engine import ip_attention
    B, N, H, DP = Q.shape
    ns = K.shape[0]
    HD = H * DP
    q2, o2, k2 = Q.reshape(B * N, HD), O.reshape(B * N, HD), K.reshape(ns * 16, HD)
    vt2 = V.permute(2, 3, 0, 1).reshape(HD, ns * 16)
    ldq, ldo, ldvt = ldq or HD, ldo or HD, ldvt or ns * 16
    if guard:
        qd, kd, vd = poisoned(q2.to(DEV), ldq), poisoned(k2.to(DEV), HD + 8), poisoned(vt2.to(DEV), ldvt)
        big, od = guarded((B * N, HD), torch.bfloat16, ldo, fill="bytes", device=DEV)
        od.copy_(o2)
    else:
        def wide(t, ld):
            buf = torch.full((t.shape[0], ld), float("nan"), dtype=torch.bfloat16, device=DEV)
            buf[:, :t.shape[1]] = t
            return buf[:, :t.shape[1]]
        qd, kd, vd, od, big = wide(q2, ldq), wide(k2, HD), wide(vt2, ldvt), wide(o2, ldo), None
    ip_attention(qd, kd, vd, od, slots, counts, scales, H, N, DP)
    return od.cpu().reshape(B, N, H, DP), (big, od)


@pytest.mark.parametrize("N,H,d,DP,T", R.OP_CASES, ids=[f"N{c[0]}-H{c[1]}-d{c[2]}to{c[3]}-T{c[4]}" for c in R.OP_CASES])
def test_op_matches_the_fp64_restatement(N, H, d, DP, T):
    """Every element within the derived bar of O + sigma softmax(Q Kip^T) Vip in fp64: B = 3 with slots [1, -1, 0] and scales [0.6, ., -0.5],
    ldq / ldo / ldvt larger than the packed widths, Q at twice the unit score gain; the key rows behind the count hold large values (a
    kernel that scores them is far off); the skipped stream keeps its bytes."""
    Q, K, V, O = R.op_inputs(N, H, d, DP, T)
    counts = [T, 1, T]
    got, _ = _launch(Q, K, V, O, R.OP_SLOTS, counts, R.OP_SCALES, ldq=H * DP + 8, ldo=H * DP + 16, ldvt=16 * R.NSLOT + 8)
    ref, bar = R.op_ref(Q, K, V, O, R.OP_SLOTS, counts, R.OP_SCALES)
    worst, share = R.worst_and_share(got, ref, bar)
    print(f"ip_attention N {N} H {H} d {d} -> DP {DP} T {T}: worst |got - ref| / bar = {worst:.3f}")
    assert bool(torch.isfinite(got.float()).all())
    assert worst <= 1.0, share
    assert torch.equal(got[1].view(torch.int16), O[1].view(torch.int16))
    assert torch.equal(got[..., d:].view(torch.int16), O[..., d:].view(torch.int16))            # pad columns keep their value
    assert not torch.equal(got[0], O[0]) and not torch.equal(got[2], O[2])
    far, share_missing = R.worst_and_share(O[..., :d], ref[..., :d], bar[..., :d])               # the input itself (no image term) is far outside
    assert share_missing > 0.5, (far, share_missing)


@pytest.mark.parametrize("N,H,d,DP,T", [(24, 3, 80, 96, 3), (1008, 2, 64, 64, 4), (1024, 2, 64, 64, 16)])
def test_op_is_batch_invariant_and_deterministic(N, H, d, DP, T):
    """Stream k of a launch of seven equals the same stream launched alone, bit for bit, and a second run equals the first."""
    Q, K, V, O = R.op_inputs(N, H, d, DP, T, B=7, nslot=3)
    slots, counts, scales = [0, 1, 2, -1, 1, 0, 2], [T, 1, T, T, T, max(1, T - 1), T], [1.0, 0.5, -0.7, 1.0, 0.25, 2.0, 0.0]
    a, _ = _launch(Q, K, V, O, slots, counts, scales)
    b, _ = _launch(Q, K, V, O, slots, counts, scales)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    for k in (0, 2, 4, 5):
        one, _ = _launch(Q[k:k + 1], K, V, O[k:k + 1], slots[k:k + 1], counts[k:k + 1], scales[k:k + 1])
        assert torch.equal(one[0].view(torch.int16), a[k].view(torch.int16)), k
        assert not torch.equal(a[k], O[k])
    for k in (3, 6):
        assert torch.equal(a[k].view(torch.int16), O[k].view(torch.int16)), k


def test_op_memory_contract():
    """Q, O, Kip and VTip inside guarded / poisoned windows, N = 24 (a tail tile), DP = 96: the guards of O stay intact, the padding columns
    of the inputs (NaN) are never read, pad columns d .. DP of O keep their value, everything is finite and meets the bar."""
    N, H, d, DP, T = 24, 3, 80, 96, 3
    Q, K, V, O = R.op_inputs(N, H, d, DP, T)
    counts = [T, 1, T]
    got, (big, od) = _launch(Q, K, V, O, R.OP_SLOTS, counts, R.OP_SCALES, ldq=H * DP + 8, ldo=H * DP + 24, ldvt=16 * R.NSLOT + 16, guard=True)
    assert intact(big, od), damage(big, od)
    assert bool(torch.isfinite(got.float()).all())
    ref, bar = R.op_ref(Q, K, V, O, R.OP_SLOTS, counts, R.OP_SCALES)
    assert R.worst_and_share(got, ref, bar)[0] <= 1.0
    assert torch.equal(got[..., d:].view(torch.int16), O[..., d:].view(torch.int16))
    assert torch.equal(got[1].view(torch.int16), O[1].view(torch.int16))


def test_op_refuses_what_it_cannot_do():
    from rich_text_to_image_amd.engine import RtError
    Q, K, V, O = R.op_inputs(8, 1, 8, 32, 1)
    for counts, scales in (([0, 1, 1], R.OP_SCALES), ([17, 1, 1], R.OP_SCALES), ([1, 1, 1], (float("nan"), 0.0, 1.0)), ([1, 1, 1], (1.0, float("inf"), 1.0))):
        with pytest.raises(RtError) as e:
            _launch(Q, K, V, O, R.OP_SLOTS, counts, scales)
        assert e.value.code == -1
    with pytest.raises(RtError):                                     # N % 8
        _launch(Q[:, :4], K, V, O[:, :4], R.OP_SLOTS, [1, 1, 1], R.OP_SCALES)


# ---------------------------------------------------------------------------------------------------------------- the forward
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


def _forward(eng, c):
    x = torch.cat([c["lat"], c["lat"], c["lat_ref"], c["lat"]]).to(DEV)
    return eng.unet_forward(x, c["t"], [0, 2, 2, 1], fontsize=[0, 1, 0, 0], qk_src=[0, 1, 2, 2], res_src=[-1, -1, -1, 2]).cpu()


def _ip_case(which, T):
    """forward_case + the adapter's weights and two images A (base / text_ref: prompt slot 2) and B (the injected region: slot 1)."""
    c = dict(forward_case(which))
    c["sd_ip"] = dict(c["sd"]); c["sd_ip"].update(R.ip_weights(c["sd"], 5))
    g = torch.Generator().manual_seed(77 + T)
    D = c["cfg"]["cross_attention_dim"]
    c["A"], c["B"] = torch.randn(T, D, generator=g), torch.randn(T, D, generator=g)
    return c


def _tokens(c, T, entries):
    """[3, T, D] for the three prompt slots from {slot: [t <= T, D]}; rows past an entry's own tokens hold NaN-free noise the count hides."""
    tk = torch.full((3, T, c["cfg"]["cross_attention_dim"]), 3.0)
    for s, t in entries.items():
        tk[s, :t.shape[0]] = t
    return tk.to(DEV)


@pytest.mark.parametrize("which,T", [("xl", 4), ("xl", 16), ("sd", 4), ("sd", 16)])
def test_forward_with_stream_modes_matches_the_ip_oracle(which, T):
    """One batched forward of uncond / base + font size / text_ref / injected region; base and text_ref carry image A, the region image B,
    both at scale 1, the uncond stream none: every stream within the project's forward bar of the oracle with the image term plugged
    in.  (The two CPU oracles alone, on these inputs: the one with the images is 0.075 - 0.26 from the one without, so a dropped term
    fails the bar by 5 x or more; the test asserts at least 3 x.)  A slot with count 3 < T matches the oracle given 3 tokens."""
    c = _ip_case(which, T)
    eng = _engine(c["cfg"], c["h"], c["w"], c["sd_ip"], ip_tokens=T)
    try:
        _set_prompts(eng, c)
        eng.set_image_prompts(_tokens(c, T, {2: c["A"], 1: c["B"]}), [0.0, 1.0, 1.0])
        got = _forward(eng, c)
        ref = oracle_streams(R.IpOracleUNet(c["cfg"], c["sd_ip"], [(None, 0.0), (c["A"], 1.0), (c["A"], 1.0), (c["B"], 1.0)]), c)
        plain = oracle_streams(OracleUNet(c["cfg"], c["sd"]), c)
        for k, name in enumerate(("uncond", "base+fontsize", "text_ref", "region injected")):
            r, d = rel_l2(got[k], ref[k]), rel_l2(ref[k], plain[k])
            print(f"{which} T {T} stream {name}: rel-L2 vs IP oracle {r:.3e}; IP oracle vs plain oracle {d:.3e}")
            assert r < FORWARD_BAR, name
            assert (d > 3 * FORWARD_BAR) == (k > 0), name             # (a property of the two CPU oracles: a dropped term cannot pass the bar)
        alone = eng.unet_forward(c["lat"].to(DEV), c["t"], [2], fontsize=[1]).cpu()          # batch invariance, bit for bit
        assert torch.equal(alone[0], got[1])
        # count 3 < T on slot 2: the oracle given the first 3 tokens of A
        eng.set_image_prompts(_tokens(c, T, {2: c["A"][:3], 1: c["B"]}), [0.0, 1.0, 1.0], counts=[T, T, 3])
        got3 = _forward(eng, c)
        ref3 = oracle_streams(R.IpOracleUNet(c["cfg"], c["sd_ip"], [(None, 0.0), (c["A"][:3], 1.0), (c["A"][:3], 1.0), (c["B"], 1.0)]), c)
        for k in (1, 2):
            assert rel_l2(got3[k], ref3[k]) < FORWARD_BAR, k
        assert torch.equal(got3[0], got[0])                  # (the injected region reads text_ref's attn1 and resnet feature: it moves too)
        assert rel_l2(got3[3], ref3[3]) < FORWARD_BAR
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- steps
def _rich_case(hw=32, R_=3, steps=3, seed=77, T=4):
    cfg = TINY_XL_CONFIG
    g = torch.Generator().manual_seed(seed)
    sched = OracleEuler(); sched.set_timesteps(steps)
    sd = random_state_dict(cfg, seed=12)
    sd_ip = dict(sd); sd_ip.update(R.ip_weights(sd, 5))
    D = cfg["cross_attention_dim"]
    c = dict(cfg=cfg, sd=sd, sd_ip=sd_ip, hw=hw, steps=steps, sched=sched, T=T,
             emb=torch.randn(R_ + 1, 77, D, generator=g), pooled=torch.randn(R_ + 1, 32, generator=g),
             tid=torch.tensor([[hw * 8.0, hw * 8.0, 0, 0, hw * 8.0, hw * 8.0]]),
             masks=torch.softmax(torch.randn(R_, 1, hw, hw, generator=g) * 2, 0).repeat(1, 4, 1, 1),
             lat=torch.randn(1, 4, hw, hw, generator=g) * sched.init_noise_sigma, gs=5.0, isa=0.5, ibg=0.4)
    c["A"], c["B"] = torch.randn(T, D, generator=g), torch.randn(T, D, generator=g)
    # prompt slots [negative, region 0, region 1, base]: the base image A on slot 3, region 0's image B on slot 1
    c["tokens"] = torch.stack([torch.zeros(T, D), c["B"], torch.zeros(T, D), c["A"]])
    c["scales"] = [0.0, 0.8, 0.0, 1.0]
    return c


def _rich_setup(eng, c, images=True):
    eng.set_prompts(c["emb"].to(DEV), c["pooled"].to(DEV), c["tid"])
    eng.set_masks(c["masks"].to(DEV))
    eng.set_fontsize(torch.tensor([3, 5]), torch.tensor([4.0, -2.0]))
    if images:
        eng.set_image_prompts(c["tokens"].to(DEV), c["scales"])


def _rich_reset(eng, c):
    eng.set_schedule(0, c["sched"].timesteps.tolist(), c["sched"].sigmas.tolist(), c["steps"])
    eng.set_latents(c["lat"].to(DEV))


def _rich_loop(eng, c):
    _rich_reset(eng, c)
    for i in range(c["steps"]):
        eng.region_step(i, c["gs"], c["isa"], c["ibg"], xl=True)
    return eng.read_latents(c["hw"], c["hw"], with_ref=True)


@pytest.fixture(scope="module")
def rich():
    c = _rich_case()
    eng = _engine(c["cfg"], c["hw"], c["hw"], c["sd_ip"], ip_tokens=c["T"])
    _rich_setup(eng, c)
    yield c, eng
    eng.close()


def test_off_is_off():
    """An engine with ip_tokens = 4 and no image prompt set, and one whose scales are all 0 (with and without tokens), give torch.equal
    outputs to an engine with ip_tokens = 0: on unet_forward with all four stream modes and on three region_steps.  set_prompts after
    set_image_prompts switches the images off again."""
    fc = _ip_case("xl", 4)
    c = _rich_case()
    plain_f = _engine(fc["cfg"], fc["h"], fc["w"], fc["sd"])
    try:
        _set_prompts(plain_f, fc)
        want_f = _forward(plain_f, fc)
    finally:
        plain_f.close()
    plain_s = _engine(c["cfg"], c["hw"], c["hw"], c["sd"])
    try:
        _rich_setup(plain_s, c, images=False)
        want_s = _rich_loop(plain_s, c)
    finally:
        plain_s.close()
    eng = _engine(fc["cfg"], fc["h"], fc["w"], fc["sd_ip"], ip_tokens=4)
    try:
        _set_prompts(eng, fc)
        assert torch.equal(_forward(eng, fc), want_f)                                       # nothing set
        eng.set_image_prompts(_tokens(fc, 4, {2: fc["A"], 1: fc["B"]}), [0.0, 0.0, 0.0])
        assert torch.equal(_forward(eng, fc), want_f)                                       # every scale 0
        eng.set_image_prompts(None, [0.0, 0.0, 0.0])
        assert torch.equal(_forward(eng, fc), want_f)
        eng.set_image_prompts(_tokens(fc, 4, {2: fc["A"], 1: fc["B"]}), [0.0, 1.0, 1.0])
        on = _forward(eng, fc)
        assert torch.equal(on[0], want_f[0]) and all(rel_l2(on[k], want_f[k]) > 5 * FORWARD_BAR for k in (1, 2, 3))
        _set_prompts(eng, fc)                                                               # set_prompts resets the scales
        assert torch.equal(_forward(eng, fc), want_f)
    finally:
        eng.close()
    eng = _engine(c["cfg"], c["hw"], c["hw"], c["sd_ip"], ip_tokens=4)
    try:
        _rich_setup(eng, c, images=False)
        got = _rich_loop(eng, c)
        assert torch.equal(got[0], want_s[0]) and torch.equal(got[1], want_s[1])
        eng.set_image_prompts(c["tokens"].to(DEV), [0.0] * 4)
        got = _rich_loop(eng, c)
        assert torch.equal(got[0], want_s[0]) and torch.equal(got[1], want_s[1])
        eng.set_image_prompts(c["tokens"].to(DEV), c["scales"])
        got = _rich_loop(eng, c)
        assert rel_l2(got[0].cpu(), want_s[0].cpu()) > 1e-2
    finally:
        eng.close()


def _ip_schedule(c, prompts):
    """(tokens, scale) of each oracle forward from the prompt slot it runs."""
    return [(c["tokens"][p] if c["scales"][p] != 0 else None, c["scales"][p]) for p in prompts]


def test_region_step_matches_the_composition_of_ip_oracle_forwards(rich):
    """The injected first region_step (7 streams: uncond, base, uncond_ref, text_ref, three regions) with a base image and one region
    image: both latent streams after the scheduler step against rich_step_forwards on the IP oracle, on the latent UPDATE."""
    c, eng = rich
    R_ = c["masks"].shape[0]
    _rich_reset(eng, c)
    eng.region_step(0, c["gs"], c["isa"], 0.0, xl=True)
    got, got_ref = (t.cpu() for t in eng.read_latents(c["hw"], c["hw"], with_ref=True))
    sched, lat0, gs = c["sched"], c["lat"], c["gs"]
    t = sched.timesteps[0]
    assert float(t) > (1 - c["isa"]) * 1000
    # forwards of rich_step_forwards: uncond (slot 0), base (R), uncond_ref (0), text_ref (R), regions (1 .. R - 1)
    o = R.IpOracleUNet(c["cfg"], c["sd_ip"], _ip_schedule(c, [0, R_, 0, R_] + list(range(1, R_))))

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
    ref, ref_ref = compose(o)
    pl, pl_ref = compose(OracleUNet(c["cfg"], c["sd"]))
    r, rr = rel_l2(got - lat0, ref - lat0), rel_l2(got_ref - lat0, ref_ref - lat0)
    d, dr = rel_l2(pl - lat0, ref - lat0), rel_l2(pl_ref - lat0, ref_ref - lat0)
    print(f"region_step with image prompts: latent UPDATE rel-L2 {r:.3e} (reference stream {rr:.3e}); the oracle without images is {d:.3e} / {dr:.3e} away")
    assert r < STEP_BAR and rr < STEP_BAR
    assert d > 3 * STEP_BAR and dr > 3 * STEP_BAR


def test_plain_step_matches_the_composition_of_ip_oracle_forwards():
    """plain_step (streams [uncond = slot 0, text = slot 1]) with an image on the text prompt."""
    c = _rich_case()
    eng = _engine(c["cfg"], c["hw"], c["hw"], c["sd_ip"], ip_tokens=c["T"])
    try:
        emb, pooled = c["emb"][[0, 3]], c["pooled"][[0, 3]]
        eng.set_prompts(emb.to(DEV), pooled.to(DEV), c["tid"])
        eng.set_image_prompts(torch.stack([torch.zeros_like(c["A"]), c["A"]]).to(DEV), [0.0, 1.0])
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
    ref = compose(R.IpOracleUNet(c["cfg"], c["sd_ip"], [(None, 0.0), (c["A"], 1.0)]))
    pl = compose(OracleUNet(c["cfg"], c["sd"]))
    r, d = rel_l2(got - lat0, ref - lat0), rel_l2(pl - lat0, ref - lat0)
    print(f"plain_step with an image prompt: latent UPDATE rel-L2 {r:.3e}; the oracle without the image is {d:.3e} away")
    assert r < STEP_BAR
    assert d > 3 * STEP_BAR


def test_split_step_equals_the_whole_step_with_image_prompts(rich):
    """rt_region_step_part for both parts of two, then _finish, gives the bits of rt_region_step: a stream uses the image of the prompt
    it runs, whichever rank runs it."""
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


def test_region_step_with_image_prompts_is_hipgraph_capturable(rich):
    """As test_region_step_is_hipgraph_capturable (tests/test_engine_gpu.py) with image prompts set: nothing is allocated and nothing
    synchronises inside the step (slots, counts and scales travel in the kernel arguments), and the replay gives the eager step's bits."""
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


def test_the_image_term_is_profiled_under_its_own_class(rich):
    c, eng = rich
    _rich_reset(eng, c)
    eng.profile_enable(True)
    eng.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True)
    eng.synchronize()
    ip = eng.profile_read_ip()
    eng.profile_enable(False)
    n_attn2 = len(R.attn2_names(c["cfg"]))
    assert ip["launches"] == n_attn2 and ip["total_bytes"] > 0 and ip["total_ms"] > 0, ip


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_engine_usable(rich):
    """RT_E_INVALID for a call on an ip_tokens = 0 engine, count 0 or 17 (or above ip_tokens), a NaN scale, n_prompts too large, NULL
    tokens with a scale set; the state is unchanged: the next forward keeps its bits."""
    from rich_text_to_image_amd.engine import RtError
    import ctypes as C
    c, eng = rich
    x = c["lat"].to(DEV)
    before = eng.unet_forward(x, 500.0, [3]).cpu()
    tk = c["tokens"].to(DEV)
    bad = [dict(tokens=tk, scales=c["scales"], counts=[0, 1, 1, 1]), dict(tokens=tk, scales=c["scales"], counts=[1, 17, 1, 1]),
           dict(tokens=tk, scales=c["scales"], counts=[1, 1, c["T"] + 1, 1]), dict(tokens=tk, scales=[0.0, float("nan"), 0.0, 1.0]),
           dict(tokens=tk, scales=[0.0, float("inf"), 0.0, 1.0]), dict(tokens=None, scales=c["scales"]),
           dict(tokens=torch.cat([tk, tk[:1]]), scales=c["scales"] + [1.0])]
    for kw in bad:
        with pytest.raises(RtError) as e:
            eng.set_image_prompts(**kw)
        assert e.value.code == -1, kw
        assert torch.equal(eng.unet_forward(x, 500.0, [3]).cpu(), before)
    assert eng.lib.rt_set_image_prompts(eng.h, C.c_void_p(tk.data_ptr()), None, None, 4) == -1          # NULL scales
    assert torch.equal(eng.unet_forward(x, 500.0, [3]).cpu(), before)
    off = _engine(c["cfg"], c["hw"], c["hw"], c["sd"])
    try:
        _rich_setup(off, c, images=False)
        want = off.unet_forward(x, 500.0, [3]).cpu()
        for kw in (dict(tokens=None, scales=[0.0] * 4), dict(tokens=tk, scales=c["scales"])):
            off.ip_tokens = c["T"]                                   # (past the binding's own shape check: the refusal under test is the library's)
            with pytest.raises(RtError) as e:
                off.set_image_prompts(**kw)
            assert e.value.code == -1
            assert torch.equal(off.unet_forward(x, 500.0, [3]).cpu(), want)
    finally:
        off.close()
    with pytest.raises(RtError):
        _engine(c["cfg"], c["hw"], c["hw"], c["sd"], ip_tokens=17)


# ---------------------------------------------------------------------------------------------------------------- projection and facade
def test_projection_matches_its_fp64_restatement():
    """project(): LayerNorm(Linear(e).reshape(T, D)) through rt_op_small_linear / rt_op_layernorm against fp64 on the bf16 weights: one
    bf16 rounding of the result (2^-8 relative) plus the fp32 arithmetic in front of it."""
    from rich_text_to_image_amd.ip_adapter import load_ip_adapter, project
    cfg = TINY_XL_CONFIG
    ck, _ = R.synthetic_checkpoint(cfg, random_state_dict(cfg, seed=12), T=4, E=24)
    ad = load_ip_adapter(ck, cfg)
    e = torch.randn(24, generator=torch.Generator().manual_seed(2))
    got = project(ad, e).cpu()
    proj = dict(ad["image_proj"]); proj["proj.weight"] = proj["proj.weight"].to(torch.bfloat16).float()
    ref = R.project_ref(proj, e)
    assert got.shape == (4, cfg["cross_attention_dim"])
    assert ((got.double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-4).all()


def _facade(which, c, adapter=None):
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    from rich_text_to_image_amd.region_diffusion_sdxl import RegionDiffusionXL
    m = RegionDiffusionXL(device=0, unet_state_dict=c["sd"], config=c["cfg"]) if which == "xl" else RegionDiffusion(0, unet_state_dict=c["sd"], config=c["cfg"])
    m.masks = [c["masks"][r:r + 1] for r in range(c["masks"].shape[0])]
    if adapter is not None:
        m.load_ip_adapter(adapter)
    return m


def test_facade_xl_equals_a_hand_driven_engine_loop_and_clear_restores_the_bits():
    """tiny XL: load_ip_adapter(state_dict) + set_image_prompts(base=, regions={0:}) through sample(run_rich_text=True) equals the same
    steps driven by hand on an engine, differs from the run without images, and clear_image_prompts() restores the bits of a pipeline
    that never loaded an adapter."""
    from rich_text_to_image_amd.ip_adapter import load_ip_adapter, project
    c = _rich_case()
    hw, R_ = c["hw"], c["masks"].shape[0]
    ck, _ = R.synthetic_checkpoint(c["cfg"], c["sd"], T=4, E=24, seed=5)
    g = torch.Generator().manual_seed(4)
    eA, tB = torch.randn(24, generator=g), torch.randn(3, c["cfg"]["cross_attention_dim"], generator=g)
    tfd = {"word_pos": torch.tensor([3, 5]), "font_size": torch.tensor([4.0, -2.0])}

    def sample(m):
        return m.sample(prompt=None, height=8 * hw, width=8 * hw, num_inference_steps=3, guidance_scale=c["gs"], latents=c["lat"].clone() / c["sched"].init_noise_sigma,
                        prompt_embeds=c["emb"][1:], negative_prompt_embeds=c["emb"][:1], pooled_prompt_embeds=c["pooled"][1:],
                        negative_pooled_prompt_embeds=c["pooled"][:1], output_type="latent", run_rich_text=True, text_format_dict=tfd,
                        inject_selfattn=c["isa"], inject_background=c["ibg"]).images.cpu()
    never = sample(_facade("xl", c))
    m = _facade("xl", c, ck)
    assert torch.equal(sample(m), never)                             # an adapter without image prompts: off is off
    m.set_image_prompts(base=dict(embeds=eA, scale=0.9), regions={0: dict(tokens=tB, scale=0.7)})
    on = sample(m)
    assert rel_l2(on, never) > 1e-2
    assert torch.equal(sample(m), on)
    with pytest.raises(ValueError):                                  # region 2 of a request with two region prompts
        m.set_image_prompts(regions={2: dict(tokens=tB)})
        sample(m)
    m.clear_image_prompts()
    assert torch.equal(sample(m), never)
    # by hand
    ad = load_ip_adapter(ck, c["cfg"])
    sd_ip = dict(c["sd"]); sd_ip.update(ad["weights"])
    eng = _engine(c["cfg"], hw, hw, sd_ip, ip_tokens=4)
    try:
        eng.set_prompts(c["emb"].to(DEV), c["pooled"].to(DEV), c["tid"])
        tokens = torch.zeros(R_ + 1, 4, c["cfg"]["cross_attention_dim"], device=DEV)
        tokens[R_] = project(ad, eA)
        tokens[1, :3] = tB.to(DEV)
        eng.set_image_prompts(tokens, [0.0, 0.7] + [0.0] * (R_ - 2) + [0.9], counts=[4, 3] + [4] * (R_ - 1))
        eng.set_masks(c["masks"].to(DEV))
        eng.set_fontsize(tfd["word_pos"], tfd["font_size"])
        # the facade's own tables and start: the caller's latents times init_noise_sigma, on the device (xl.py:533-536)
        m.scheduler.set_timesteps(3)
        eng.set_schedule(m.scheduler.kind, m.scheduler.timesteps.tolist(), m.scheduler.table(), 3)
        eng.set_latents((c["lat"].clone() / c["sched"].init_noise_sigma).to(DEV).float() * m.scheduler.init_noise_sigma)
        for i in range(3):
            eng.region_step(i, c["gs"], c["isa"], c["ibg"], xl=True)
        hand = eng.read_latents(hw, hw).cpu()
    finally:
        eng.close()
    assert torch.equal(hand, on)


def test_facade_sd_prompt_to_img_path_with_image_prompts():
    """tiny SD: produce_latents (the rich pass of prompt_to_img) and plain_latents with image prompts differ from the run without, repeat
    bit for bit, and clear_image_prompts() restores the bits of a pipeline that never loaded an adapter."""
    from oracle.schedulers import OraclePNDM
    cfg = TINY_SD_CONFIG
    g = torch.Generator().manual_seed(31)
    hw, R_ = 32, 3
    c = dict(cfg=cfg, sd=random_state_dict(cfg, seed=12), masks=torch.softmax(torch.randn(R_, 1, hw, hw, generator=g) * 2, 0).repeat(1, 4, 1, 1))
    emb = torch.randn(R_ + 1, 77, cfg["cross_attention_dim"], generator=g)
    lat = torch.randn(1, 4, hw, hw, generator=g)
    ck, _ = R.synthetic_checkpoint(cfg, c["sd"], T=4, E=24, seed=5, layout="diffusers")
    eA, eB = torch.randn(24, generator=g), torch.randn(24, generator=g)

    def rich(m):
        return m.produce_latents(emb, height=8 * hw, width=8 * hw, num_inference_steps=3, guidance_scale=7.5, latents=lat.clone(),
                                 inject_selfattn=0.5, inject_background=0.4).cpu()

    def plain(m):
        return m.plain_latents(emb[[0, R_]], 8 * hw, 8 * hw, 3, 7.5, lat.clone()).cpu()
    m0 = _facade("sd", c)
    never_r, never_p = rich(m0), plain(m0)
    m = _facade("sd", c, ck)
    m.set_image_prompts(base=dict(embeds=eA), regions={1: dict(embeds=eB, scale=0.6)})
    on_r, on_p = rich(m), plain(m)
    assert rel_l2(on_r, never_r) > 1e-2 and rel_l2(on_p, never_p) > 1e-2
    assert torch.equal(rich(m), on_r) and torch.equal(plain(m), on_p)
    m.set_image_prompts(regions={1: dict(embeds=eB, scale=0.6)})     # no base image: the plain pass is text-only again
    assert torch.equal(plain(m), never_p) and not torch.equal(rich(m), never_r)
    m.clear_image_prompts()
    assert torch.equal(rich(m), never_r) and torch.equal(plain(m), never_p)
    m.unload_ip_adapter()
    assert torch.equal(rich(m), never_r)


def test_facade_sd_prompt_to_img_equals_a_hand_driven_engine_loop():
    """tiny SD with a tokenizer, a text encoder and a VAE (tests/test_sample_gpu.py's model): load_ip_adapter(state_dict) +
    set_image_prompts(base=, regions={1:}) through prompt_to_img / produce_latents (rich pass) and plain_latents equals the same steps
    driven by hand on an Engine built with ip_tokens = T - prompt slots [negative, region 0, region 1, base], the region image on slot 2 with
    its own count and scale, the base image on the last slot, set right after set_prompts - bit for bit; it differs from the run without
    images and from the hand loop with the region image on the other region's slot; clear_image_prompts() restores the bits of the
    pipeline before it loaded an adapter."""
    from rich_text_to_image_amd.ip_adapter import load_ip_adapter, project
    from rich_text_to_image_amd.schedulers import PNDMTables
    from tests.test_sample_gpu import _model
    m = _model()
    cfg, sd = TINY_SD_CONFIG, random_state_dict(TINY_SD_CONFIG, seed=1)          # _model()'s UNet weights
    D = cfg["cross_attention_dim"]
    n, gs, h, w, isa, ibg, R_ = 4, 7.5, 64, 64, 0.5, 0.5, 3
    g = torch.Generator().manual_seed(8)
    lat = torch.randn(1, 4, h, w, generator=g)
    masks = torch.softmax(torch.randn(R_, 1, h, w, generator=g) * 2, 0).repeat(1, 4, 1, 1)
    m.masks = [masks[r:r + 1] for r in range(R_)]
    prompts, neg = ["a wooden fence covered in snow", "a red barn", "a barn and a fence under a night sky"], ""
    kw = dict(num_inference_steps=n, guidance_scale=gs, inject_selfattn=isa, inject_background=ibg)
    emb = m.get_text_embeds(prompts, [neg])                          # [negative, region 0, region 1, base]
    assert emb.shape[0] == R_ + 1
    never_img = m.prompt_to_img(prompts, neg, latents=lat.clone(), **kw)
    never_lat = m.produce_latents(emb, latents=lat.clone(), **kw).cpu()
    never_plain = m.plain_latents(emb[[0, R_]], num_inference_steps=n, guidance_scale=gs, latents=lat.clone()).cpu()
    ck, _ = R.synthetic_checkpoint(cfg, sd, T=4, E=24, seed=5)
    eA, tB = torch.randn(24, generator=g), torch.randn(3, D, generator=g)
    m.load_ip_adapter(ck)
    m.set_image_prompts(base=dict(embeds=eA, scale=0.9), regions={1: dict(tokens=tB, scale=0.6)})
    img = m.prompt_to_img(prompts, neg, latents=lat.clone(), **kw)
    lat_on = m.produce_latents(emb, latents=lat.clone(), **kw).cpu()
    plain_on = m.plain_latents(emb[[0, R_]], num_inference_steps=n, guidance_scale=gs, latents=lat.clone()).cpu()
    assert (img != never_img).any() and rel_l2(lat_on, never_lat) > 1e-2 and rel_l2(plain_on, never_plain) > 1e-2
    # by hand
    ad = load_ip_adapter(ck, cfg)
    sd_ip = dict(sd); sd_ip.update(ad["weights"])
    t = PNDMTables().set_timesteps(n)
    eng = _engine(cfg, h, w, sd_ip, ip_tokens=4)
    try:
        tokA = project(ad, eA)

        def hand(emb_, slots, rich):
            """slots: {prompt slot: (tokens [t, D] on the device, scale)}"""
            P = emb_.shape[0]
            eng.set_prompts(emb_.to(DEV))
            tokens = torch.zeros(P, 4, D, device=DEV)
            counts, scales = [4] * P, [0.0] * P
            for s, (tk, sc) in slots.items():
                tokens[s, :tk.shape[0]] = tk.to(DEV)
                counts[s], scales[s] = tk.shape[0], sc
            eng.set_image_prompts(tokens, scales, counts=counts)
            eng.set_fontsize(None, None)
            eng.set_schedule(1, t.timesteps.tolist(), t.table(), n)
            eng.set_latents(lat.to(DEV))
            if rich:
                eng.set_masks(masks.to(DEV))
            for i in range(len(t.timesteps)):
                if rich:
                    eng.region_step(i, gs, isa, ibg, xl=False)
                else:
                    eng.plain_step(i, gs)
            return eng.read_latents(h, w).cpu()
        want = hand(emb, {R_: (tokA, 0.9), 2: (tB, 0.6)}, True)
        assert torch.equal(lat_on, want)
        assert (img == m.latents_to_uint8(want.to(DEV))).all()
        assert torch.equal(plain_on, hand(emb[[0, R_]], {1: (tokA, 0.9)}, False))
        # what the comparison would catch: the region image on region 0's slot, a dropped scale
        assert not torch.equal(hand(emb, {R_: (tokA, 0.9), 1: (tB, 0.6)}, True), want)
        assert not torch.equal(hand(emb, {R_: (tokA, 0.9), 2: (tB, 1.0)}, True), want)
    finally:
        eng.close()
    m.clear_image_prompts()
    assert torch.equal(m.produce_latents(emb, latents=lat.clone(), **kw).cpu(), never_lat)
    assert (m.prompt_to_img(prompts, neg, latents=lat.clone(), **kw) == never_img).all()
