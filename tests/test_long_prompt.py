"""Prompts longer than one 77-token CLIP window, CPU side: the chunking rule (clip_tokenizer.encode_chunks), the position of a base
token among the concatenated windows (chunk_key), the rich-text front end on a text of ~100 tokens, and the encoders' output layout
(zero-padded embeddings + key counts).  Synthetic BPE vocabulary as in tests/test_text_side.py."""
import json
import types

import pytest
import torch


@pytest.fixture(scope="module")
def tok(tmp_path_factory):
    from rich_text_to_image_amd import clip_tokenizer as ct
    d = tmp_path_factory.mktemp("vocab_long")
    alpha = list(ct._byte_alphabet().values())
    vocab = alpha + [a + "</w>" for a in alpha]
    merges = [("c", "a"), ("ca", "t</w>"), ("t", "h"), ("th", "e</w>"), ("d", "o"), ("do", "g</w>"), ("i", "n"), ("in", "g</w>"),
              ("r", "u"), ("ru", "n"), ("n", "ing</w>")]
    vocab += [a + b for a, b in merges] + ["<|startoftext|>", "<|endoftext|>"]
    json.dump({t: i for i, t in enumerate(vocab)}, open(d / "vocab.json", "w"))
    open(d / "merges.txt", "w").write("#version: 0.2\n" + "\n".join(a + " " + b for a, b in merges) + "\n")
    json.dump({"pad_token": "!"}, open(d / "special_tokens_map.json", "w"))          # a pad id that is not EOS (SDXL's second tokenizer)
    return ct.ClipBPETokenizer.from_pretrained(str(d))


def _text(n):
    """n BPE tokens: 'cat' is one token of the stub vocabulary"""
    return " ".join(["cat"] * n)


@pytest.mark.parametrize("n,chunks", [(0, 1), (75, 1), (76, 2), (150, 2), (151, 3), (225, 3)])
def test_chunk_counts_and_row_layout(tok, n, chunks):
    from rich_text_to_image_amd import clip_tokenizer as ct
    # distinct inner ids, so that the concatenation check sees order and loss: dog / the / cat cycle
    words = [("cat", "dog", "the")[i % 3] for i in range(n)]
    text = " ".join(words)
    ids = tok.convert_tokens_to_ids(tok._tokenize(text))
    assert len(ids) == n and ct.chunk_count(n) == chunks
    rows = ct.encode_chunks(tok, text, 3)
    assert len(rows) == chunks
    inner = []
    for r in rows:
        assert len(r) == 77 and r[0] == tok.bos_token_id
        k = r.index(tok.eos_token_id)
        assert 1 <= k <= 76 and all(v == tok.pad_token_id for v in r[k + 1:])
        assert tok.bos_token_id not in r[1:k] and tok.eos_token_id not in r[1:k]
        inner += r[1:k]
    assert inner == ids
    assert all(len(r) - 2 - r[r.index(tok.eos_token_id) + 1:].count(tok.pad_token_id) == 75 for r in rows[:-1])      # only the last window is short
    assert tok.encode_chunks(text, 3) == rows


def test_too_long_is_an_error_never_a_silent_cut(tok):
    from rich_text_to_image_amd import clip_tokenizer as ct
    with pytest.raises(ValueError, match=r"226 tokens.*max_prompt_chunks=3"):
        ct.encode_chunks(tok, _text(226), 3)
    with pytest.raises(ValueError, match=r"76 tokens.*max_prompt_chunks=1"):
        ct.encode_chunks(tok, _text(76), 1)
    with pytest.raises(ValueError):
        ct.encode_chunks(tok, _text(3), 4)
    # one window of a text that fits = today's truncating call, id for id
    for n in (0, 1, 40, 75):
        assert ct.encode_chunks(tok, _text(n), 1) == [tok.encode(_text(n), 77, True, "max_length")]


def test_key_mapping():
    from rich_text_to_image_amd.clip_tokenizer import chunk_key
    assert [chunk_key(i) for i in (0, 74, 75, 149, 150)] == [1, 75, 78, 152, 155]
    assert [chunk_key(i) for i in range(75)] == list(range(1, 76))                       # today's i + 1 inside the first window
    keys = [chunk_key(i) for i in range(225)]
    assert len(set(keys)) == 225 and max(keys) == 229 and not any(k % 77 in (0, 76) for k in keys)


class _RecordingEncoder:
    """text_encoder(ids)[0]: embeds every id as a constant row, so that outputs can be traced back to the ids; records its inputs"""

    def __init__(self, D=8):
        self.D, self.seen = D, []

    def __call__(self, ids):
        self.seen.append(ids.clone())
        return (ids.float()[..., None].repeat(1, 1, self.D) + torch.arange(ids.shape[1]).float()[None, :, None] / 1000.0,)


def _sd_facade(tok, enc, **kw):
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    from oracle.unet import TINY_SD_CONFIG
    m = RegionDiffusion(device=0, unet_state_dict={}, config=TINY_SD_CONFIG, tokenizer=tok, text_encoder=enc, **kw)      # no engine is built here
    m.device = torch.device("cpu")
    return m


def test_default_facade_sends_todays_truncated_ids_and_opt_in_sends_windows(tok):
    long, short = _text(60) + " dog " + _text(39), "the dog"                           # 100 tokens / 2 tokens
    enc = _RecordingEncoder()
    m = _sd_facade(tok, enc)
    emb = m.get_text_embeds([long], [""])
    assert torch.is_tensor(emb) and emb.shape == (2, 77, 8)
    today = tok([long], padding="max_length", max_length=77, truncation=True, return_tensors="pt").input_ids
    assert torch.equal(enc.seen[0], today) and today[0, -1] == tok.eos_token_id        # cut at 75 tokens, as before
    lst = m.get_text_embeds_list([long, short])
    assert isinstance(lst, list) and all(e.shape == (1, 77, 8) for e in lst)

    enc2 = _RecordingEncoder()
    m2 = _sd_facade(tok, enc2, max_prompt_chunks=2)
    emb2, counts = m2.get_text_embeds([long, short], [""])
    assert counts == [77, 154, 77] and emb2.shape == (3, 154, 8)
    assert not emb2[0, 77:].any() and not emb2[2, 77:].any() and emb2[1, 77:].abs().sum() > 0      # zero rows past a prompt's own keys
    rows = enc2.seen[0]
    assert rows.shape == (4, 77)                                                        # every window is a 77-token row of its own
    assert rows.tolist() == [tok.encode_chunks("", 2)[0]] + tok.encode_chunks(long, 2) + tok.encode_chunks(short, 2)
    # a short prompt's window = what the default path encodes
    assert torch.equal(emb2[2, :77], m.get_text_embeds([short], [""])[1])
    # the per-call argument overrides the constructor's; too long for the limit is an error
    e3, c3 = m.get_text_embeds([long], [""], max_prompt_chunks=3)
    assert c3 == [77, 154] and e3.shape == (2, 154, 8)
    with pytest.raises(ValueError, match="160 tokens"):
        m2.get_text_embeds([_text(160)], [""])
    lst2, c4 = m2.get_text_embeds_list([long, short])
    assert c4 == [154, 77] and [tuple(e.shape) for e in lst2] == [(1, 154, 8), (1, 77, 8)]


def _rich_model(tok, max_prompt_chunks=2):
    return types.SimpleNamespace(tokenizer=tok, max_prompt_chunks=max_prompt_chunks)


def test_rich_text_positions_after_token_75(tok):
    """~100-token base text with a size span, a colour span and a footnote target behind token 75: every id list and word_pos uses the
    mapped key positions, the background list holds mapped positions of unused tokens only (no BOS / EOS / pad key)."""
    from rich_text_to_image_amd import richtext_utils as ru
    from rich_text_to_image_amd.clip_tokenizer import chunk_key
    js = {"ops": [{"insert": _text(90) + " the "}, {"attributes": {"size": "60px"}, "insert": "dog"}, {"insert": " "},
                  {"attributes": {"color": "#ff0000"}, "insert": "running"}, {"insert": " "},
                  {"attributes": {"link": "the cat"}, "insert": "7"}, {"insert": " 4 2\n"}]}
    base, styles, notes, note_tok, color_p, color_names, color_rgbs, sizes, guid = ru.parse_json(js, device="cpu")
    model = _rich_model(tok)
    prompts, ids, base_tokens = ru.get_region_diffusion_input(model, base, styles, notes, note_tok, color_p, color_names)
    n = len(base_tokens)
    assert 95 <= n <= 110 and base_tokens[:90] == ["cat</w>"] * 90
    i_dog, i_run, i_ning, i_7 = (base_tokens.index(t) for t in ("dog</w>", "run", "ning</w>", "7</w>"))
    assert min(i_dog, i_run, i_ning, i_7) > 75
    assert prompts == ["the cat", "red running", base]
    assert ids[0].tolist() == [chunk_key(i_7)] and ids[1].tolist() == [chunk_key(i_run), chunk_key(i_ning)]
    assert min(ids[0].tolist() + ids[1].tolist()) >= 78
    bg = ids[2].tolist()
    last = n - 75                                                                      # tokens in the second window
    assert not any(k % 77 in (0, 76) for k in bg)                                      # no BOS / EOS position
    assert all(k < 77 or 1 <= k - 77 <= last for k in bg)                              # no pad position of the last window
    assert sorted(bg) == sorted(chunk_key(i) for i in range(n) if i not in (i_7, i_run, i_ning))
    tfd = ru.get_attention_control_input(model, base_tokens, sizes, device="cpu")
    assert tfd["word_pos"].tolist() == [chunk_key(i_dog)] and tfd["word_pos"][0] >= 78 and tfd["font_size"].tolist() == [20.0]
    tfd, cids = ru.get_gradient_guidance_input(model, base_tokens, color_p, color_rgbs, tfd)
    assert cids[0].tolist() == [chunk_key(i_run), chunk_key(i_ning)]
    assert sorted(cids[1].tolist()) == sorted(chunk_key(i) for i in range(n) if i not in (i_run, i_ning))
    # the recorded cross map of this text has 154 columns: every id indexes it
    assert max(max(g.tolist()) for g in ids + cids) < 154


def test_a_span_behind_the_allowed_windows_is_refused_by_name(tok):
    """Default (one window): a formatted word behind token 75 has no key.  The front end says so - token count and max_prompt_chunks in
    the message - instead of handing out a position past the 77 columns; an unformatted tail is dropped from the background list as
    its encoding is cut."""
    from rich_text_to_image_amd import richtext_utils as ru
    js = {"ops": [{"insert": _text(90) + " the "}, {"attributes": {"size": "60px"}, "insert": "dog"}, {"insert": " 4 2\n"}]}
    base, styles, notes, note_tok, color_p, color_names, color_rgbs, sizes, guid = ru.parse_json(js, device="cpu")
    for model in (_rich_model(tok, 1), types.SimpleNamespace(tokenizer=tok)):
        prompts, ids, base_tokens = ru.get_region_diffusion_input(model, base, styles, notes, note_tok, color_p, color_names)
        assert ids[-1].tolist() == list(range(1, 76))
        with pytest.raises(ValueError, match=rf"{len(base_tokens)} tokens.*max_prompt_chunks=1"):
            ru.get_attention_control_input(model, base_tokens, sizes, device="cpu")
    tfd = ru.get_attention_control_input(_rich_model(tok, 1), base_tokens, sizes, device="cpu", max_prompt_chunks=2)      # the call's own choice wins
    assert tfd["word_pos"].tolist()[0] >= 78


def test_clip_encoders_xl_chunked_layout(tok):
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
    from rich_text_to_image_amd.checkpoint import ClipEncodersXL
    torch.manual_seed(0)
    n_vocab = len(tok.encoder)
    kw = dict(vocab_size=n_vocab, intermediate_size=64, num_attention_heads=2, max_position_embeddings=77, eos_token_id=tok.eos_token_id,
              bos_token_id=tok.bos_token_id, pad_token_id=tok.pad_token_id)
    e1 = CLIPTextModel(CLIPTextConfig(hidden_size=32, num_hidden_layers=3, **kw))
    e2 = CLIPTextModelWithProjection(CLIPTextConfig(hidden_size=48, num_hidden_layers=2, projection_dim=40, **kw))
    enc = ClipEncodersXL([tok, tok], [e1, e2], torch.device("cpu"))
    short, long = "the dog", _text(50) + " dog " + _text(49)
    pe, ne, pp, npool, pc, nc = enc([short, long], [""], max_prompt_chunks=2)
    assert pe.shape == (2, 154, 80) and pc == [77, 154] and ne.shape == (1, 154, 80) and nc == [77]
    assert not pe[0, 77:].any() and not ne[0, 77:].any() and pe[1, 77:].abs().sum() > 0
    assert pp.shape == (2, 40) and npool.shape == (1, 40)
    rows = torch.tensor(tok.encode_chunks(short, 2) + tok.encode_chunks(long, 2))
    with torch.no_grad():
        o1, o2 = e1(rows, output_hidden_states=True), e2(rows, output_hidden_states=True)
    hid = torch.cat([o1.hidden_states[-2], o2.hidden_states[-2]], -1)
    assert torch.allclose(pe[0, :77], hid[0], atol=1e-6) and torch.allclose(pe[1], hid[1:3].reshape(154, 80), atol=1e-6)
    assert torch.allclose(pp[0], o2[0][0], atol=1e-6) and torch.allclose(pp[1], o2[0][1], atol=1e-6)      # pooled: window 0 of encoder 2
    assert not torch.allclose(pp[1], o2[0][2], atol=1e-4)
    # zeroed negative (xl.py:363-366) keeps its meaning; the default call is untouched
    pe0, ne0, pp0, np0, pc0, nc0 = enc([long], None, max_prompt_chunks=3)
    assert pe0.shape == (1, 154, 80) and not ne0.any() and not np0.any() and nc0 == [77]
    four = enc([short, long], [""])
    assert len(four) == 4 and four[0].shape == (2, 77, 80)
    with pytest.raises(ValueError, match="tokens"):
        enc([_text(151)], [""], max_prompt_chunks=2)


def test_cli_and_requests_carry_max_prompt_chunks(tmp_path):
    from rich_text_to_image_amd import sample
    a = sample.build_parser().parse_args(["--rich_text_json", '{"ops":[{"insert":"a cat\\n"}]}', "--max_prompt_chunks", "3"])
    assert a.max_prompt_chunks == 3
    assert [r["max_prompt_chunks"] for r in sample.build_requests(a)] == [3]
    assert sample.build_parser().parse_args(["--rich_text_json", "{}"]).max_prompt_chunks == 1
    f = tmp_path / "reqs.jsonl"
    f.write_text('{"rich_text_json": {"ops": [{"insert": "a\\n"}]}, "max_prompt_chunks": 2}\n{"rich_text_json": {"ops": [{"insert": "b\\n"}]}}\n')
    a = sample.build_parser().parse_args(["--requests", str(f)])
    assert [r["max_prompt_chunks"] for r in sample.build_requests(a)] == [2, 1]
    with pytest.raises(SystemExit):
        sample.build_parser().parse_args(["--rich_text_json", "{}", "--max_prompt_chunks", "4"])


def test_a_refused_engine_request_leaves_the_limits():
    """HipUNet2DConditionModel.engine checks every request before it moves a limit: a call refused for its stream count does not leave
    max_keys grown without an engine built for it."""
    from rich_text_to_image_amd.unet import HipUNet2DConditionModel
    m = HipUNet2DConditionModel({"in_channels": 4}, state_dict="random0")
    before = (m.max_streams, m.max_prompts, m.max_keys)
    with pytest.raises(ValueError, match="16"):
        m.engine(8, 8, streams=17, prompts=20, keys=154)
    with pytest.raises(ValueError, match="77, 154 or 231"):
        m.engine(8, 8, prompts=20, keys=100)
    assert (m.max_streams, m.max_prompts, m.max_keys) == before
