"""Self-contained CLIP byte-pair tokenizer.

The reference leans on transformers 4.27's slow `CLIPTokenizer._tokenize` (utils/richtext_utils.py:150,160,171,195,220),
which later transformers releases dropped.  This is the published CLIP BPE algorithm (OpenAI `simple_tokenizer.py`; the
HF slow tokenizer without ftfy lower-cases and collapses whitespace) over a checkpoint's own `vocab.json` + `merges.txt`
- neither file is available offline, so tests use a synthetic vocabulary and, where transformers can build a tokenizer
from the same files, compare against it.  [memory] parity unpinned against transformers 4.27.
"""
import json
import os
from functools import lru_cache
from types import SimpleNamespace

import regex
import torch

_PAT = regex.compile(r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+", regex.IGNORECASE)


@lru_cache()
def _byte_alphabet():
    """GPT-2 reversible byte<->printable-unicode table: printable latin-1 bytes map to themselves, the rest to 256+k."""
    keep = list(range(ord('!'), ord('~') + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    table, extra = {}, 0
    for b in range(256):
        if b in keep:
            table[b] = chr(b)
        else:
            table[b] = chr(256 + extra)
            extra += 1
    return table


# ---- prompts longer than one CLIP window: 77-id windows of [BOS] + <= 75 ids + [EOS] + pad, encoded one by one and concatenated
CHUNK_TOKENS = 75          # BPE ids per window
CHUNK_KEYS = 77            # cross-attention keys per window: BOS, the ids, EOS / pad
MAX_PROMPT_CHUNKS = 3


def chunk_count(n_tokens):
    """Windows a text of n_tokens BPE ids (without BOS / EOS) needs: 0, 75 -> 1; 76, 150 -> 2; 151, 225 -> 3."""
    return max(1, -(-n_tokens // CHUNK_TOKENS))


def chunk_key(i):
    """Key position of base token i (0-based, without BOS) in the concatenated windows: i + 1 inside the first window, then past
    every window's EOS and the next one's BOS.  0 -> 1, 74 -> 75, 75 -> 78, 149 -> 152, 150 -> 155."""
    return CHUNK_KEYS * (i // CHUNK_TOKENS) + 1 + i % CHUNK_TOKENS


def check_max_prompt_chunks(max_chunks):
    if max_chunks not in (1, 2, 3):
        raise ValueError(f"max_prompt_chunks must be 1, 2 or 3, got {max_chunks!r}")
    return max_chunks


def encode_chunks(tokenizer, text, max_chunks=MAX_PROMPT_CHUNKS):
    """The 77-id rows of `text`: its BPE ids split every 75 (no look-back to commas, no weighting syntax), each row
    [BOS] + <= 75 ids + [EOS] + pad with the tokenizer's own pad id.  A text that needs more than `max_chunks` rows raises ValueError:
    nothing is cut silently.  Works with any tokenizer that has tokenize / _tokenize, convert_tokens_to_ids and the three special ids."""
    check_max_prompt_chunks(max_chunks)
    tokenize = getattr(tokenizer, "_tokenize", None) or tokenizer.tokenize
    ids = list(tokenizer.convert_tokens_to_ids(tokenize(text)))
    n = chunk_count(len(ids))
    if n > max_chunks:
        raise ValueError(f"prompt of {len(ids)} tokens needs {n} windows of {CHUNK_TOKENS}; max_prompt_chunks={max_chunks} allows "
                         f"{max_chunks * CHUNK_TOKENS} tokens: {text[:60]!r}...")
    rows = []
    for c in range(n):
        inner = ids[c * CHUNK_TOKENS:(c + 1) * CHUNK_TOKENS]
        row = [tokenizer.bos_token_id] + inner + [tokenizer.eos_token_id]
        rows.append(row + [tokenizer.pad_token_id] * (CHUNK_KEYS - len(row)))
    return rows


def encode_text_chunked(tokenizers, encode_rows, texts, max_chunks):
    """Shared by the two facades.  texts -> (embeddings [P, 77 c_max, D] with zero rows behind a prompt's own windows, key counts [P],
    extra): every window goes through `encode_rows(k, ids [n, 77]) -> (hidden [n, 77, D_k], extra_k [n, ...] or None)` of tokenizer /
    encoder k as a 77-token row of its own; hidden states are concatenated on channels over k and on rows over a prompt's windows;
    `extra` is the last encoder's extra output of every prompt's FIRST window (SDXL's pooled embedding)."""
    import torch
    per_tok = [[encode_chunks(tok, t, max_chunks) for t in texts] for tok in tokenizers]
    nchunks = [len(r) for r in per_tok[0]]
    for rows in per_tok[1:]:                     # SDXL's tokenizers share the vocabulary; only the pad id differs
        if [len(r) for r in rows] != nchunks:
            raise ValueError("the tokenizers disagree on the number of windows of a prompt")
    hidden, extra = [], None
    for k, rows in enumerate(per_tok):
        flat = torch.tensor([row for r in rows for row in r], dtype=torch.long)
        h, x = encode_rows(k, flat)
        hidden.append(h.float())
        extra = x
    hid = torch.cat(hidden, dim=-1)                                   # [sum chunks, 77, D]
    cmax, first = max(nchunks), 0
    out = hid.new_zeros(len(texts), CHUNK_KEYS * cmax, hid.shape[-1])
    firsts = []
    for p, n in enumerate(nchunks):
        out[p, :CHUNK_KEYS * n] = hid[first:first + n].reshape(CHUNK_KEYS * n, -1)
        firsts.append(first)
        first += n
    counts = [CHUNK_KEYS * n for n in nchunks]
    return out, counts, (extra[firsts].float() if extra is not None else None)


def pad_keys(emb, length):
    """[P, L, D] -> [P, length, D] with zero rows appended (prompt sets of different window counts share one tensor)."""
    import torch
    if emb.shape[1] == length:
        return emb
    return torch.cat([emb, emb.new_zeros(emb.shape[0], length - emb.shape[1], emb.shape[2])], 1)


class ClipBPETokenizer:
    model_max_length = 77

    def __init__(self, vocab_file, merges_file, pad_token=None, bos_token="<|startoftext|>", eos_token="<|endoftext|>"):
        self.encoder = json.load(open(vocab_file, encoding="utf-8"))
        self.decoder = {v: k for k, v in self.encoder.items()}
        lines = open(merges_file, encoding="utf-8").read().strip().split("\n")[1:49152 - 256 - 2 + 1]
        self.ranks = {tuple(l.split()): i for i, l in enumerate(lines) if l}
        self.bos_token, self.eos_token = bos_token, eos_token
        self.pad_token = pad_token if pad_token is not None else eos_token
        self.bos_token_id = self.encoder[bos_token]
        self.eos_token_id = self.encoder[eos_token]
        self.pad_token_id = self.encoder[self.pad_token]
        self._cache = {bos_token: bos_token, eos_token: eos_token}

    @classmethod
    def from_pretrained(cls, path, subfolder=None):
        d = os.path.join(path, subfolder) if subfolder else path
        pad = None
        sp = os.path.join(d, "special_tokens_map.json")
        if os.path.exists(sp):
            pt = json.load(open(sp)).get("pad_token")
            pad = pt.get("content") if isinstance(pt, dict) else pt
        return cls(os.path.join(d, "vocab.json"), os.path.join(d, "merges.txt"), pad_token=pad)

    def _bpe(self, token):
        if token in self._cache:
            return self._cache[token]
        word = list(token[:-1]) + [token[-1] + "</w>"]
        while len(word) > 1:
            best = min(zip(word, word[1:]), key=lambda p: self.ranks.get(p, float("inf")))
            if best not in self.ranks:
                break
            a, b = best
            merged, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == a and word[i + 1] == b:
                    merged.append(a + b)
                    i += 2
                else:
                    merged.append(word[i])
                    i += 1
            word = merged
        out = " ".join(word)
        self._cache[token] = out
        return out

    def _tokenize(self, text):
        text = " ".join(text.split()).strip().lower()
        alphabet = _byte_alphabet()
        pieces = []
        for tok in regex.findall(_PAT, text):
            tok = "".join(alphabet[b] for b in tok.encode("utf-8"))
            pieces.extend(self._bpe(tok).split(" "))
        return pieces

    tokenize = _tokenize

    def convert_tokens_to_ids(self, tokens):
        unk = self.encoder[self.eos_token]
        return [self.encoder.get(t, unk) for t in tokens]

    def encode(self, text, max_length=None, truncation=False, padding=None):
        ids = [self.bos_token_id] + self.convert_tokens_to_ids(self._tokenize(text)) + [self.eos_token_id]
        max_length = max_length or self.model_max_length
        if truncation and len(ids) > max_length:
            ids = ids[:max_length - 1] + [self.eos_token_id]
        if padding == "max_length":
            ids = ids + [self.pad_token_id] * (max_length - len(ids))
        return ids

    def encode_chunks(self, text, max_chunks=MAX_PROMPT_CHUNKS):
        return encode_chunks(self, text, max_chunks)

    def __call__(self, text, padding=None, max_length=None, truncation=False, return_tensors=None, **_):
        texts = [text] if isinstance(text, str) else list(text)
        rows = [self.encode(t, max_length, truncation, padding) for t in texts]
        if return_tensors == "pt":
            width = max(len(r) for r in rows)
            rows = [r + [self.pad_token_id] * (width - len(r)) for r in rows] if padding else rows
            return SimpleNamespace(input_ids=torch.tensor(rows, dtype=torch.long))
        return SimpleNamespace(input_ids=rows if not isinstance(text, str) else rows[0])
