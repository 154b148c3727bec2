"""Request isolation at the engine level: the jobs whose result must be a function of the job alone ("probes"), the jobs that run before
them on the same engine ("histories"), and the two ways a probe prepares a used engine.  Test infrastructure for
tests/test_request_isolation_gpu.py; every "returns it to its default" call below is taken from the state inventory in INTEGRATION.md
("State that outlives a run") and from nowhere else.

  probe      inputs(eng, c, last)  the job's own inputs: prompts, masks, font sizes, schedule, latents.  `last` names which of the two
                                   calls that reset the solver state comes last ("latents": set_schedule then set_latents; "schedule":
                                   the other order) - each alone must do.
             run(eng, c)           the steps -> an ordered dict of named tensors (with_ref returns two streams: "latents" first)
  history    run(eng, c, o)        a dirty job on case `o` (other prompts, masks, latents); returns the inventory items it leaves away from
                                   their default that NO input call of a probe brings back ("prediction", "freeu", "source", "store", "profiling")
  explicit   every option of the inventory set to the probe's value by name, whatever ran before; the solver is reset by set_schedule
  minimal    only the inventory's clearing calls for what the histories since the last probe left; the solver is reset by set_latents
"""
import collections

import torch

from freeu_ref import FORWARD_FREEU
from ip_adapter_ref import ip_weights
from oracle.schedulers import OracleEuler, OraclePNDM
from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, random_state_dict

DEV = "cuda:0"
FU = (FORWARD_FREEU["s1"], FORWARD_FREEU["s2"], FORWARD_FREEU["b1"], FORWARD_FREEU["b2"])
ENGINE_KW = dict(xl=dict(max_streams=12, max_prompts=8, max_keys=231, ip_tokens=16), sd=dict(max_streams=12, max_prompts=8))
# the recorded modules of P4 and of the attention-store history: a self-attention and a cross-attention map of the 16 x 16 level
STORE_NAMES = dict(xl=("down_blocks.1.attentions.0.transformer_blocks.0.attn1", "down_blocks.1.attentions.0.transformer_blocks.0.attn2"),
                   sd=("down_blocks.1.attentions.0.transformer_blocks.0.attn1", "down_blocks.1.attentions.0.transformer_blocks.0.attn2"))
MAX_PROMPTS = 7                                      # the 6-region history sets 7 prompts


def make_case(which, h=32, w=32, seed=77):
    xl = which == "xl"
    cfg = TINY_XL_CONFIG if xl else TINY_SD_CONFIG
    g = torch.Generator().manual_seed(seed)
    D = cfg["cross_attention_dim"]
    sd = random_state_dict(cfg, seed=12)
    if xl:
        sd = {**sd, **ip_weights(sd, 5)}
    euler = OracleEuler(); euler.set_timesteps(3)
    c = dict(which=which, xl=xl, cfg=cfg, sd=sd, h=h, w=w, seed=seed, R=3, gs=5.0 if xl else 7.5, isa=0.5, ibg=0.4,
             emb=torch.randn(MAX_PROMPTS, 231, D, generator=g), pooled=torch.randn(MAX_PROMPTS, 32, generator=g) if xl else None,
             tid=torch.tensor([[h * 8.0, w * 8.0, 0, 0, h * 8.0, w * 8.0]]) if xl else None,
             noise=torch.randn(1, 4, h, w, generator=g), x0=torch.randn(1, 4, h, w, generator=g),
             keep=(torch.rand(h, w, generator=g) > 0.5).float(), tokens=torch.randn(MAX_PROMPTS, 16, D, generator=g),
             wp=torch.tensor([3, 5]), fs=torch.tensor([4.0, -2.0]), sigma0=euler.init_noise_sigma)
    c["masks"] = {R: torch.softmax(torch.randn(R, 1, h, w, generator=g) * 2, 0).repeat(1, 4, 1, 1) for R in (1, 3, 6)}
    return c


def build_engine(c, h=None, w=None):
    from rich_text_to_image_amd.engine import Engine
    e = Engine(c["cfg"], h or c["h"], w or c["w"], device=0, **ENGINE_KW[c["which"]])
    e.load_state_dict(c["sd"])
    assert e.weights_missing()[0] == 0
    return e


# ---------------------------------------------------------------------------------------------------------------- pieces of a job
def schedule(name, n):
    """(kind, timesteps, table, num_inference_steps) of rt_set_schedule."""
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerAncestralTables
    if name == "euler":
        s = OracleEuler(); s.set_timesteps(n)
        return 0, s.timesteps.tolist(), s.sigmas.tolist(), n
    if name == "pndm":
        s = OraclePNDM(); s.set_timesteps(n)
        return 1, s.timesteps.tolist(), s.alphas_cumprod.tolist(), n
    if name == "euler-a":
        s = EulerAncestralTables().set_timesteps(n)
        return s.kind, s.timesteps.tolist(), s.table(), n
    order, algo = {"dpm1": (1, "dpmsolver++"), "dpm2": (2, "dpmsolver++"), "sde2": (2, "sde-dpmsolver++")}[name]
    s = DPMSolverTables(solver_order=order, algorithm=algo).set_timesteps(n)
    return s.kind, s.timesteps.tolist(), s.table(), n


def sigma_space(sched):
    return sched[0] in (0, 4)


def start(eng, c, sched, last="latents"):
    lat = (c["noise"] * (c["sigma0"] if sigma_space(sched) else 1.0)).to(DEV)
    if last == "latents":
        eng.set_schedule(*sched)
        eng.set_latents(lat)
    else:
        eng.set_latents(lat)
        eng.set_schedule(*sched)


def set_text(eng, c, rows, keys=77, key_counts=None):
    emb = c["emb"][rows, :keys].contiguous().to(DEV)
    if c["xl"]:
        eng.set_prompts(emb, c["pooled"][rows].contiguous().to(DEV), c["tid"], key_counts=key_counts)
    else:
        eng.set_prompts(emb, key_counts=key_counts)


def rich_inputs(eng, c, R=None, keys=77, key_counts=None, font=True):
    """Prompts [negative, R - 1 region prompts, base], R masks and the font-size words of case c."""
    R = c["R"] if R is None else R
    set_text(eng, c, list(range(R + 1)), keys, key_counts)
    eng.set_masks(c["masks"][R].to(DEV))
    if font:
        eng.set_fontsize(c["wp"], c["fs"])
    else:
        eng.set_fontsize(None, None)


def rich_steps(eng, c, steps):
    for i in steps:
        eng.region_step(i, c["gs"], c["isa"], c["ibg"], xl=c["xl"])


def read(eng, c):
    lat, ref = eng.read_latents(c["h"], c["w"], with_ref=True)
    return collections.OrderedDict([("latents", lat), ("reference latents", ref)])


def first_difference(got, want):
    """The name of the first stream of `want` that `got` does not match bit for bit, or None."""
    for name, t in want.items():
        if not torch.equal(got[name], t):
            return name
    return None


# ---------------------------------------------------------------------------------------------------------------- the probes
class P1:
    """XL rich loop with Euler: 3 steps, R = 3, font sizes (4, -2), inject_selfattn 0.5, inject_background 0.4."""
    which, name = "xl", "P1-xl-rich-euler"

    @staticmethod
    def inputs(eng, c, last):
        rich_inputs(eng, c)
        start(eng, c, schedule("euler", 3), last)

    @staticmethod
    def run(eng, c):
        rich_steps(eng, c, range(3))
        return read(eng, c)


class P2:
    """XL plain pass with DPM-Solver++ of order 2: 3 steps on the prompts [negative, base]."""
    which, name = "xl", "P2-xl-plain-dpm2"

    @staticmethod
    def inputs(eng, c, last):
        set_text(eng, c, [0, c["R"]])
        start(eng, c, schedule("dpm2", 3), last)

    @staticmethod
    def run(eng, c):
        for i in range(3):
            eng.plain_step(i, c["gs"])
        return read(eng, c)


class P3:
    """SD rich loop with PNDM: set_timesteps(4) = 5 iterations, so the warm-up pair and the history of four are all used."""
    which, name = "sd", "P3-sd-rich-pndm"

    @staticmethod
    def inputs(eng, c, last):
        rich_inputs(eng, c)
        start(eng, c, schedule("pndm", 4), last)

    @staticmethod
    def run(eng, c):
        rich_steps(eng, c, range(5))
        return read(eng, c)


class P4:
    """P1 behind a recorded plain pass: two attention maps are enabled, 11 plain steps cross the "more than 10 calls" rule (one map is
    recorded, by call 11), the maps and their call counts are read, then P1's loop runs.  The store is part of this job: inputs() enables
    it - or, where the caller knows it was left enabled in this mode (store_left=True), only resets it, which is the inventory's
    clearing call for the counters and the maps."""
    which, name = "xl", "P4-xl-store-then-rich"

    @staticmethod
    def inputs(eng, c, last, store_left=False):
        rich_inputs(eng, c)
        if not store_left:
            for n in STORE_NAMES[c["which"]]:
                eng.attn_store_enable(n, 1)
        eng.attn_store_reset()
        start(eng, c, schedule("euler", 11), last)

    @staticmethod
    def run(eng, c):
        out = collections.OrderedDict()
        for i in range(11):
            eng.plain_step(i, c["gs"])
        for n in STORE_NAMES[c["which"]]:
            calls, m = eng.attn_store_read(n)
            out["calls of " + n] = torch.tensor(calls)
            out["map of " + n] = m
            eng.attn_store_enable(n, 0)
        start(eng, c, schedule("euler", 3), "latents")
        rich_steps(eng, c, range(3))
        out.update(read(eng, c))
        return out


PROBES = {p.name: p for p in (P1, P2, P3, P4)}


# ---------------------------------------------------------------------------------------------------------------- the two preambles
def all_modules(eng):
    return [n for n, _, _ in eng.attn_modules()]


CLEAR = {                                          # inventory item -> its documented way back to the default
    "prediction": lambda eng: eng.set_prediction(0, 0.0),
    "freeu": lambda eng: eng.disable_freeu(),
    "source": lambda eng: eng.set_source(None),
    "store": lambda eng: [eng.attn_store_enable(n, 0) for n in STORE_NAMES["xl"]],
    "profiling": lambda eng: eng.profile_enable(False),
}


def prepare(eng, c, probe, mode, dirty=()):
    """mode "fresh": the job's inputs on an engine nothing else has used.  "explicit" / "minimal": see the module docstring."""
    if mode == "fresh":
        probe.inputs(eng, c, "latents")
        return
    if mode == "explicit":
        eng.set_stream(None)
        eng.set_prediction(0, 0.0)
        eng.set_noise_seed(0)
        eng.set_freeu(1.0, 1.0, 1.0, 1.0)
        eng.set_source(None)
        eng.profile_enable(False)
        for n in all_modules(eng):
            eng.attn_store_enable(n, 0)
        eng.attn_store_reset()
        probe.inputs(eng, c, "schedule")
        if eng.ip_tokens and probe is not P2:                # by name: no prompt slot has an image (set_prompts has said so already)
            eng.set_image_prompts(None, [0.0] * (c["R"] + 1))
        elif eng.ip_tokens:
            eng.set_image_prompts(None, [0.0, 0.0])
        return
    assert mode == "minimal", mode
    store_left = probe is P4 and "store" in dirty
    for item in dirty:
        if not (item == "store" and store_left):
            CLEAR[item](eng)
    if probe is P4:
        probe.inputs(eng, c, "latents", store_left=store_left)
    else:
        probe.inputs(eng, c, "latents")


def run_probe(eng, c, probe, mode, dirty=()):
    prepare(eng, c, probe, mode, dirty)
    return probe.run(eng, c)


# ---------------------------------------------------------------------------------------------------------------- the histories
def refused(call):
    from rich_text_to_image_amd.engine import RtError
    try:
        call()
    except RtError as e:
        assert e.code == -1, e
        return
    raise AssertionError("a call that must be refused was accepted")


def h_dpm_stopped(eng, c, o):
    """A DPM-Solver++ 2 run of 3 steps stopped after its first: one x0 in the history, the slot index flipped."""
    rich_inputs(eng, o)
    start(eng, o, schedule("dpm2", 3))
    rich_steps(eng, o, [0])
    return ()


def h_pndm_in_warmup(eng, c, o):
    """A PNDM run stopped inside its warm-up pair: counter 1, one stored prediction, cur_sample held (plain pass on the XL engine, whose
    rich loop takes no PNDM; rich loop on the SD engine)."""
    if c["xl"]:
        set_text(eng, o, [0, 1])
        start(eng, o, schedule("pndm", 4))
        eng.plain_step(0, o["gs"])
    else:
        rich_inputs(eng, o)
        start(eng, o, schedule("pndm", 4))
        rich_steps(eng, o, [0])
    return ()


def h_stochastic_other_seed(eng, c, o):
    """SDE-DPM-Solver++ 2 and (sigma space: XL) Euler ancestral with noise seed 12345.  The probes are deterministic and ignore the seed."""
    eng.set_noise_seed(12345)
    rich_inputs(eng, o)
    start(eng, o, schedule("sde2", 3))
    rich_steps(eng, o, range(3))
    if c["xl"]:
        start(eng, o, schedule("euler-a", 3))
        rich_steps(eng, o, range(2))
    return ()


def h_v_prediction_rescaled(eng, c, o):
    eng.set_prediction(1, 0.7)
    rich_inputs(eng, o)
    start(eng, o, schedule("dpm1", 3))
    rich_steps(eng, o, range(2))
    return ("prediction",)


def h_freeu(eng, c, o):
    eng.set_freeu(*FU)
    rich_inputs(eng, o)
    start(eng, o, schedule("euler" if c["xl"] else "pndm", 3))
    rich_steps(eng, o, [0])
    return ("freeu",)


IP_SCALES, IP_COUNTS = [0.0, -0.6, 0.0, 0.9], [16, 4, 16, 16]


def h_image_prompts(eng, c, o):
    """16 tokens on the base slot, 4 on a region slot with a negative scale."""
    rich_inputs(eng, o)
    eng.set_image_prompts(o["tokens"][:4].to(DEV), IP_SCALES, IP_COUNTS)
    start(eng, o, schedule("euler", 3))
    rich_steps(eng, o, [0])
    return ()


def h_long_prompts(eng, c, o):
    """Prompts of 154 and of 231 keys, font-size words in the second and third window."""
    rich_inputs(eng, o, keys=154, key_counts=[77, 154, 77, 154])
    eng.set_fontsize(torch.tensor([3, 80, 150]), torch.tensor([2.0, -3.0, 5.0]))
    start(eng, o, schedule("euler", 3))
    rich_steps(eng, o, [0])
    rich_inputs(eng, o, keys=231, key_counts=[231, 154, 231, 231])
    eng.set_fontsize(torch.tensor([3, 160, 230]), torch.tensor([2.0, -3.0, 5.0]))
    start(eng, o, schedule("euler", 3))
    rich_steps(eng, o, [0])
    return ()


def h_source_kept(eng, c, o):
    """An image start with a keep mask at strength 0.5: the source, its noise and the mask stay in the engine (no set_source(None))."""
    from rich_text_to_image_amd.schedulers import EulerTables, PNDMTables
    t = (EulerTables() if c["xl"] else PNDMTables()).set_timesteps(4, 0.5)
    rich_inputs(eng, o)
    eng.set_schedule(t.kind, t.timesteps.tolist(), t.table(), 4)
    eng.set_source(o["x0"].to(DEV), o["noise"].to(DEV), o["keep"].to(DEV))
    eng.noise_latents(*t.start_level())
    levels = t.source_levels()
    for i in range(2):
        rich_steps(eng, o, [i])
        eng.source_blend(*levels[i])
    return ("source",)


def h_other_region_counts(eng, c, o):
    """One region, then six (9 streams)."""
    for R in (1, 6):
        rich_inputs(eng, o, R=R)
        start(eng, o, schedule("euler" if c["xl"] else "dpm2", 3))
        rich_steps(eng, o, [0])
    return ()


def h_other_font_words(eng, c, o):
    rich_inputs(eng, o)
    eng.set_fontsize(torch.tensor([1, 2, 7, 40]), torch.tensor([-3.0, 0.5, 6.0, 2.0]))
    start(eng, o, schedule("euler" if c["xl"] else "pndm", 3))
    rich_steps(eng, o, [0])
    return ()


def h_store_left_filled(eng, c, o):
    """The two maps of P4 enabled, filled by 11 plain steps and left as they are: enabled, counters at 11, one map recorded."""
    set_text(eng, o, [0, 1])
    for n in STORE_NAMES[c["which"]]:
        eng.attn_store_enable(n, 1)
    start(eng, o, schedule("euler" if c["xl"] else "pndm", 11))
    for i in range(11):
        eng.plain_step(i, o["gs"])
    assert eng.attn_store_read(STORE_NAMES[c["which"]][0])[0] == 11
    return ("store",)


def h_abandoned_split_step(eng, c, o):
    """region_step_part for both parts of two; region_step_finish is never called."""
    rich_inputs(eng, o)
    start(eng, o, schedule("euler" if c["xl"] else "pndm", 3))
    ranges = [eng.region_step_part(0, o["gs"], o["isa"], o["ibg"], c["xl"], part, 2)[:2] for part in (0, 1)]
    assert all(n > 0 for _, n in ranges), ranges
    return ()


def refused_calls(eng, c):
    """One refused call of every setter that validates: each raises RT_E_INVALID and, by its contract, changes nothing."""
    refused(lambda: eng.set_freeu(1.0, 1.0, 0.0, 1.0))
    refused(lambda: eng.set_freeu(float("nan"), 1.0, 1.0, 1.0))
    refused(lambda: eng.set_prediction(0, 1.5))
    refused(lambda: eng.set_prediction(2, 0.0))
    kind, ts, table, n = schedule("euler", 3)
    refused(lambda: eng.set_schedule(kind, ts, table[:-1], n))                    # Euler needs n + 1 sigmas
    kind, ts, table, n = schedule("dpm2", 3)
    refused(lambda: eng.set_schedule(kind, ts[::-1], table, n))                   # ascending timesteps
    refused(lambda: eng.set_schedule(9, ts, table, n))
    refused(lambda: eng.set_fontsize(torch.tensor([eng.max_keys]), torch.tensor([2.0])))
    if eng.ip_tokens:
        refused(lambda: eng.set_image_prompts(c["tokens"][:2].to(DEV), [0.5, 0.5], [eng.ip_tokens + 1, 1]))
        refused(lambda: eng.set_image_prompts(c["tokens"][:2].to(DEV), [float("inf"), 0.5]))
    else:
        refused(lambda: eng.set_image_prompts(None, [0.0, 0.0]))
    if eng.max_keys < 231:
        refused(lambda: eng.set_prompts(c["emb"][:2, :231].contiguous().to(DEV), key_counts=[231, 231]))


def h_refused_calls(eng, c, o):
    """A step, then the refused calls, in mid-sequence of another job."""
    rich_inputs(eng, o)
    start(eng, o, schedule("euler" if c["xl"] else "pndm", 3))
    rich_steps(eng, o, [0])
    refused_calls(eng, o)
    return ()


def h_profiling_left_on(eng, c, o):
    """Per-launch event timing switched on and left on: timing only, no result may depend on it."""
    eng.profile_enable(True)
    rich_inputs(eng, o)
    start(eng, o, schedule("euler" if c["xl"] else "pndm", 3))
    rich_steps(eng, o, [0])
    return ("profiling",)


def h_side_stream(eng, c, o):
    """A step executed on a side stream, then set_stream(None): back on the stream rt_create made."""
    rich_inputs(eng, o)
    eng.synchronize()
    side = torch.cuda.Stream()
    eng.set_stream(side.cuda_stream)
    try:
        start(eng, o, schedule("euler" if c["xl"] else "pndm", 3))
        rich_steps(eng, o, [0])
        torch.cuda.synchronize()
    finally:
        eng.set_stream(None)
    return ()


HISTORIES = collections.OrderedDict([
    ("dpm2-stopped-after-step-1", h_dpm_stopped), ("pndm-stopped-in-warmup", h_pndm_in_warmup),
    ("stochastic-other-seed", h_stochastic_other_seed), ("v-prediction-rescale-0.7", h_v_prediction_rescaled), ("freeu-on", h_freeu),
    ("image-prompts-on", h_image_prompts), ("prompts-of-154-and-231-keys", h_long_prompts), ("source-with-keep-mask", h_source_kept),
    ("regions-1-then-6", h_other_region_counts), ("other-font-size-words", h_other_font_words),
    ("attention-store-left-filled", h_store_left_filled), ("abandoned-split-step", h_abandoned_split_step),
    ("refused-setter-calls", h_refused_calls), ("profiling-left-on", h_profiling_left_on), ("step-on-a-side-stream", h_side_stream)])
XL_ONLY = ("image-prompts-on", "prompts-of-154-and-231-keys")


def histories_of(which):
    return [k for k in HISTORIES if which == "xl" or k not in XL_ONLY]


# ---------------------------------------------------------------------------------------------------------------- teeth
# An option a history turns on, still on while the probe runs: applied after the probe's inputs.  The result must differ from the fresh
# one in at least one bit, else the equalities above could hold because the option does nothing at this size.
def t_prediction(eng, c):
    eng.set_prediction(1, 0.7)


def t_freeu(eng, c):
    eng.set_freeu(*FU)


def t_image_prompts(eng, c):
    eng.set_image_prompts(c["tokens"][:4].to(DEV), IP_SCALES, IP_COUNTS)


def t_image_prompt_plain(eng, c):
    eng.set_image_prompts(c["tokens"][:2].to(DEV), [0.0, 0.9], [16, 16])


def t_font_words(eng, c):
    eng.set_fontsize(torch.tensor([1, 2, 7, 40]), torch.tensor([-3.0, 0.5, 6.0, 2.0]))


TEETH = [(P1, "prediction", t_prediction), (P1, "freeu", t_freeu), (P1, "image-prompts", t_image_prompts), (P1, "font-words", t_font_words),
         (P2, "prediction", t_prediction), (P2, "freeu", t_freeu), (P2, "image-prompts", t_image_prompt_plain),
         (P3, "prediction", t_prediction), (P3, "freeu", t_freeu), (P3, "font-words", t_font_words)]
