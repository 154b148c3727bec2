"""Reference arithmetic for prompts of more than one 77-token window (tests only).

The reference's font-size softmax (models/attention_processor.py:386-401) asserts 77 keys, and so does its restatement in
oracle/unet.py.  Chunked prompts have 77 c keys; the arithmetic itself does not depend on the count, so it is restated here without
the assert and patched over `oracle.unet.attention_probs` by the tests that need it (pytest's monkeypatch)."""
import torch


def attention_probs(q, k, scale, fontsize=None):
    """oracle.unet.attention_probs for any key count.  q, k: [B*H, N, d] / [B*H, NK, d]; fontsize: word_pos (< NK) and font_size."""
    scores = scale * torch.bmm(q, k.transpose(-1, -2))
    if fontsize is None:
        return scores.softmax(dim=-1)
    wp = fontsize["word_pos"]
    assert int(wp.max()) < k.shape[1]
    e = (scores - scores.max(-1, True)[0]).float().exp()
    e[:, :, wp] = e[:, :, wp].clone() * fontsize["font_size"].abs()
    p = e / e.sum(-1, True)
    p[:, :, wp] *= fontsize["font_size"].sign()
    return p
