"""Recorders of the two fixtures that pin the engine's host code (csrc/engine.hip) across a refactor (test infrastructure):

  layouts()     the ordered weight table, trace modules and attention modules of every (configuration, options) pair - no GPU needed;
                tests/golden/engine_layout.json, reproduced by tests/test_engine_layout.py
  on_digests()  sha256 of the outputs of the optional paths switched ON - ControlNet, image prompts, regional LoRA, the LayerNorm fold, the
                token-map store -, the host-computed profile counters and the arena sizes; tests/golden/engine_on_bits.json, reproduced
                by tests/test_engine_on_bits_gpu.py

Both fixtures are recorded on the PARENT of the commit they guard, never on the tree under test: build the parent's librtdiff.so, point
RTDIFF_LIB_PATH at it and run `python tests/engine_golden.py layout|bits <parent commit> <output.json>`.  Only Python API that the parent
has is used."""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LAYOUT_JSON = os.path.join(HERE, "golden", "engine_layout.json")
BITS_JSON = os.path.join(HERE, "golden", "engine_on_bits.json")

OPTIONS = (("none", {}), ("controlnet", dict(controlnet={})), ("ip", dict(ip_tokens=4)), ("lora", dict(lora_rank=32)),
           ("all", dict(controlnet={}, ip_tokens=4, lora_rank=32)))
FULL_LISTS = ("tiny_xl", "tiny_sd", "fold")          # stored entry by entry; the full-size ones as counts + a digest


def _configs():
    from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG
    from rich_text_to_image_amd.engine import SD15_CONFIG, SDXL_CONFIG
    from weight_influence_ref import FOLD_CONFIG
    return (("tiny_xl", TINY_XL_CONFIG), ("tiny_sd", TINY_SD_CONFIG), ("fold", FOLD_CONFIG), ("sd15", SD15_CONFIG), ("sdxl", SDXL_CONFIG))


def _canonical(lay):
    return json.dumps(lay, sort_keys=True, separators=(",", ":")).encode()


def layout_of(cfg, **opts):
    """A weight-table-only engine's layout, every list in the engine's own order: weights 'name d0xd1..', trace 'name channels shift',
    attn 'name type heads'."""
    from rich_text_to_image_amd.engine import Engine
    eng = Engine(cfg, 64, 64, device=-1, **opts)
    try:
        return dict(weights=[f"{n} {'x'.join(str(d) for d in s)}" for n, s in eng.weight_table()],
                    trace=[f"{n} {c} {s}" for n, c, s in eng.trace_modules()],
                    attn=[f"{n} {a} {b}" for n, a, b in eng.attn_modules()])
    finally:
        eng.close()


def layout_entry(cname, oname):
    """What the fixture stores under 'cname/oname'."""
    lay = layout_of(dict(_configs())[cname], **dict(OPTIONS)[oname])
    if cname not in FULL_LISTS:
        lay = dict(weights=len(lay["weights"]), trace=len(lay["trace"]), attn=len(lay["attn"]), sha256=hashlib.sha256(_canonical(lay)).hexdigest())
    return lay


def layout_keys():
    return [f"{cname}/{oname}" for cname in ("tiny_xl", "tiny_sd", "fold", "sd15", "sdxl") for oname, _ in OPTIONS]


def layouts():
    return {key: layout_entry(*key.split("/")) for key in layout_keys()}


# The file keeps the full lists in a compact form: every distinct entry once, in a table whose strings are front-coded ("<n>:<rest>" = the
# first n characters of the entry before + rest; neighbours share most of their module path), and every list as runs [first, count] of
# consecutive table indices.  The options only insert or append slots, so a list is a handful of runs.  unpack(pack(x)) == x.
def pack(lays):
    table, index, out, prev = [], {}, {}, ""
    for key in sorted(lays, key=lambda k: (k.split("/")[0], k.split("/")[1] != "all")):      # a configuration's longest lists first
        out[key] = {}
        for name, val in lays[key].items():
            if not isinstance(val, list):
                out[key][name] = val
                continue
            runs = []
            for s in val:
                if s not in index:
                    n = len(os.path.commonprefix([prev, s]))
                    index[s] = len(table); table.append(f"{n}:{s[n:]}"); prev = s
                if runs and runs[-1][0] + runs[-1][1] == index[s]:
                    runs[-1][1] += 1
                else:
                    runs.append([index[s], 1])
            out[key][name] = runs
    return table, {k: out[k] for k in lays}


def unpack(table, packed):
    entries, prev = [], ""
    for t in table:
        n, rest = t.split(":", 1)
        prev = prev[:int(n)] + rest
        entries.append(prev)
    return {key: {name: [entries[i] for a, c in val for i in range(a, a + c)] if isinstance(val, list) else val for name, val in lay.items()}
            for key, lay in packed.items()}


def load_layouts():
    with open(LAYOUT_JSON) as f:
        doc = json.load(f)
    return doc["parent"], unpack(doc["entries"], doc["layouts"])


def first_difference(got, want):
    """A line that names the first entry of the first list that differs (or the digest), for the assertion message."""
    for key in ("weights", "trace", "attn"):
        g, w = got[key], want[key]
        if isinstance(w, int):
            if g != w:
                return f"{key}: {g} entries, recorded {w}"
            continue
        for i, (a, b) in enumerate(zip(g, w)):
            if a != b:
                return f"{key}[{i}]: got '{a}', recorded '{b}'"
        if len(g) != len(w):
            return f"{key}: {len(g)} entries, recorded {len(w)}"
    return None if got.get("sha256") == want.get("sha256") else "same counts, another order or shape (sha256 of the canonical JSON)"


# ---------------------------------------------------------------------------------------------------------------- bits with the options on
def _digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _counters(eng):
    """(count, total_flops, total_bytes) of every profile class 0 - 9: computed on the host from the launches' shapes (total_ms is not)."""
    out = {}
    for cls in range(10):
        n, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
        eng._chk(eng.lib.rt_profile_read2(eng.h, cls, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)))
        out[str(cls)] = [n.value, fl.value, by.value]
    return out


def _engine(cfg, h, w, sd, **kw):
    from rich_text_to_image_amd.engine import Engine
    e = Engine(cfg, h, w, device=0, **kw)
    e.load_state_dict(sd)
    assert e.weights_missing()[0] == 0
    return e


def on_digests(device="cuda:0"):
    import torch
    import controlnet_ref as R
    import ip_adapter_ref as IP
    import regional_lora_ref as L
    from oracle.schedulers import OracleEuler
    from oracle.unet import random_state_dict
    from rich_text_to_image_amd.regional_lora import parse_adapter
    from weight_influence_ref import FOLD_CONFIG, FOLD_LATENT
    CN = dict(embed_channels=R.TINY_EMBED)
    out = {}

    # ---- the controlled forward of tests/test_controlnet_gpu.py and three of its trace points
    for which in ("xl", "sd"):
        c = R.control_case(which)
        eng = _engine(c["cfg"], c["h"], c["w"], c["sd_cn"], controlnet=CN)
        try:
            out[f"arena_forward_{which}"] = eng.arena()[1]
            if c["xl"]:
                eng.set_prompts(c["emb"].to(device), c["pooled"].to(device), c["tid"])
            else:
                eng.set_prompts(c["emb"].to(device))
            eng.set_fontsize(c["wp"], c["fs"])
            eng.set_control_hint(c["hint"].to(device))
            eng.set_control_scales(R.FORWARD_SLOT_SCALES)
            x = torch.cat([c["lat"], c["lat"], c["lat_ref"], c["lat"]]).to(device)
            kw = dict(fontsize=[0, 1, 0, 0], qk_src=[0, 1, 2, 2], res_src=[-1, -1, -1, 2])
            out[f"forward_{which}"] = _digest(eng.unet_forward(x, c["t"], R.FORWARD_STREAM_SLOTS, **kw))
            last_skip = max((n for n, _, _ in eng.trace_modules() if n.startswith("controlnet.skip.")), key=lambda n: int(n.rsplit(".", 1)[1]))
            for name in ("controlnet.conv_in", last_skip, "controlnet.mid"):
                o, t = eng.unet_forward(x, c["t"], R.FORWARD_STREAM_SLOTS, trace=name, **kw)
                out[f"forward_{which} traced {name}"] = _digest(t)
                out[f"forward_{which} output of the forward traced at {name}"] = _digest(o)
        finally:
            eng.close()

    # ---- controlled region steps: step 0 is injected, steps 1 and 2 are past the injection threshold
    c = R.rich_case()
    eng = _engine(c["cfg"], c["hw"], c["hw"], c["sd_cn"], controlnet=CN)
    try:
        out["arena_region_steps"] = eng.arena()[1]
        eng.set_prompts(c["emb"].to(device), c["pooled"].to(device), c["tid"])
        eng.set_masks(c["masks"].to(device))
        eng.set_fontsize(torch.tensor([3, 5]), torch.tensor([4.0, -2.0]))
        eng.set_control_hint(c["hint"].to(device))
        eng.set_control_scales(R.STEP_SLOT_SCALES)
        eng.set_schedule(0, c["sched"].timesteps.tolist(), c["sched"].sigmas.tolist(), c["steps"])
        eng.set_latents(c["lat"].to(device))
        assert float(c["sched"].timesteps[0]) > (1 - c["isa"]) * 1000 > float(c["sched"].timesteps[1])
        for i in range(c["steps"]):
            if i == 0:
                eng.profile_enable(True)
            eng.region_step(i, c["gs"], c["isa"], c["ibg"], xl=True)
            if i == 0:
                eng.synchronize()
                out["counters_region_step_0"] = _counters(eng)
                eng.profile_enable(False)
            lat, ref = eng.read_latents(c["hw"], c["hw"], with_ref=True)
            out[f"region_step_{i}_latents"], out[f"region_step_{i}_reference_latents"] = _digest(lat), _digest(ref)
    finally:
        eng.close()

    # ---- ControlNet + image prompts + regional LoRA together at the widths where every LayerNorm consumer takes the folded form.
    # Prompt slots 0 .. 3: LoRA (A, B) / image prompt / control - slot 0 nothing, 1 LoRA + image, 2 LoRA + control, 3 image + control.
    # Streams: 0 plain (slot 0), 1 font size (slot 1), 2 the source stream on its own latent (slot 2), 3 attends with stream 2's Q / K and
    # takes its resnet feature (slot 3).
    cfg, (h, w) = FOLD_CONFIG, FOLD_LATENT
    sd = random_state_dict(cfg, seed=4)
    ckA, _ = L.synthetic_adapter(sd, rank=4, alpha=2.0, seed=1, gain=2.0)
    ckB, _ = L.synthetic_adapter(sd, rank=8, seed=2, layout="peft")
    adapters = {"A": parse_adapter(sd, ckA)[0], "B": parse_adapter(sd, ckB)[0]}
    sd_all = {**sd, **IP.ip_weights(sd, 5), **R.prefixed(R.control_state_dict(cfg, seed=21))}
    g = torch.Generator().manual_seed(8)
    emb = torch.randn(4, 77, cfg["cross_attention_dim"], generator=g)
    lat, lat_ref = torch.randn(1, 4, h, w, generator=g), torch.randn(1, 4, h, w, generator=g)
    tokens = torch.randn(4, 4, cfg["cross_attention_dim"], generator=g)
    eng = _engine(cfg, h, w, sd_all, controlnet=CN, ip_tokens=4, lora_rank=32, max_streams=4, max_prompts=4)
    try:
        out["arena_all_three"] = eng.arena()[1]
        eng.bind_regional_loras(adapters)
        eng.set_prompts(emb.to(device))
        eng.set_fontsize(torch.tensor([2, 6]), torch.tensor([3.0, -1.5]))
        eng.set_image_prompts(tokens.to(device), [0.0, 1.0, 0.0, 0.8], counts=[4, 3, 4, 4])
        eng.set_control_hint(R.make_hint(h, w).to(device))
        eng.set_control_scales([0.0, 0.0, 1.0, 0.5])
        eng.set_lora_scales([(0.0, 0.0), (0.7, 0.0), (0.5, 0.8), (0.0, 0.0)])
        x = torch.cat([lat, lat, lat_ref, lat]).to(device)
        eng.profile_enable(True)
        got = eng.unet_forward(x, 500.0, [0, 1, 2, 3], fontsize=[0, 1, 0, 0], qk_src=[0, 1, 2, 2], res_src=[-1, -1, -1, 2])
        eng.synchronize()
        out["counters_all_three"] = _counters(eng)
        eng.profile_enable(False)
        out["all_three_forward"] = _digest(got)
        out["all_three_stream_2_alone"] = _digest(eng.unet_forward(lat_ref.to(device), 500.0, [2]))
    finally:
        eng.close()

    # ---- the token-map store: 12 plain steps of tiny XL with every map enabled (accumulating and overwriting ones alternate), so that the
    # "more than 10 calls" rule and the statistics hand-over of the eleventh and twelfth call run
    c = R.rich_case()
    sched = OracleEuler(); sched.set_timesteps(12)
    eng = _engine(c["cfg"], c["hw"], c["hw"], c["sd"])
    try:
        out["arena_store"] = eng.arena()[1]
        eng.set_prompts(c["emb"][[0, 3]].to(device), c["pooled"][[0, 3]].to(device), c["tid"])
        names = [m[0] for m in eng.attn_modules()]
        for k, n in enumerate(names):
            eng.attn_store_enable(n, 1 + k % 2)
        eng.set_schedule(0, sched.timesteps.tolist(), sched.sigmas.tolist(), 12)
        eng.set_latents((c["lat"] / c["sched"].init_noise_sigma * sched.init_noise_sigma).to(device))
        for i in range(12):
            eng.plain_step(i, c["gs"])
        out["store_latents"] = _digest(eng.read_latents(c["hw"], c["hw"]))
        for n in names:
            calls, m = eng.attn_store_read(n)
            assert calls == 12 and m is not None, (n, calls)
            out[f"store map of {n}"] = _digest(m)
    finally:
        eng.close()
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    what, parent, path = sys.argv[1:4]
    lib = os.environ.get("RTDIFF_LIB_PATH", "the tree's own librtdiff.so")
    def compact(v):
        return json.dumps(v, separators=(",", ":"))
    if what == "layout":
        lays = layouts()
        table, packed = pack(lays)
        assert unpack(table, packed) == lays
        head = {"what": "engine_golden.layouts(): the ordered weight table, trace modules and attention modules of weight-table-only engines, "
                        "packed by engine_golden.pack()", "parent": parent}
        body = ['"entries":[\n' + ",\n".join(compact(table[i:i + 24])[1:-1] for i in range(0, len(table), 24)) + "]",
                '"layouts":{\n' + ",\n".join(f"{json.dumps(k)}:{compact(v)}" for k, v in packed.items()) + "}"]
    else:
        head = {"what": "engine_golden.on_digests(): sha256 of outputs, host-computed profile counters (count, flops, bytes) and arena bytes, on an MI355X",
                "parent": parent}
        body = ['"digests":{\n' + ",\n".join(f" {json.dumps(k)}: {compact(v)}" for k, v in on_digests().items()) + "}"]
    print(f"recorded with {lib}")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("{" + ",\n".join([f"{json.dumps(k)}: {json.dumps(v)}" for k, v in head.items()] + body) + "}\n")
