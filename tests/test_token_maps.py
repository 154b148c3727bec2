"""Token-map producer: the get_token_maps port against outputs of the REFERENCE function
(tests/golden/token_maps_port.pt, oracle/make_golden.py tokenmaps) on regenerated synthetic maps -- CPU."""
import os

import torch

from oracle.synth import synthetic_attention_maps

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_get_token_maps_port_matches_reference_function():
    from rich_text_to_image_amd.attention_utils import get_token_maps
    port = torch.load(os.path.join(GOLD, "token_maps_port.pt"))
    assert len(port) == 2
    for (seed, nseg, thr), ref in port.items():
        selfm, crossm = synthetic_attention_maps(seed)
        masks = get_token_maps(selfm, crossm, {}, None, 64, 64, [torch.tensor([2, 3]), torch.tensor([6])], seed=4,
                               segment_threshold=thr, num_segments=nseg, device="cpu")
        got = torch.cat(masks)[:, 0]
        assert got.shape == ref.shape
        assert len(masks) == 3 and masks[0].shape == (1, 4, 64, 64)
        assert torch.allclose(got, ref, atol=1e-6), (got - ref).abs().max()
        assert torch.allclose(torch.cat(masks).sum(0), torch.ones(4, 64, 64), atol=1e-5)      # regions partition the image
        # the synthetic blobs are recovered: span {2,3} covers blobs 0 and 1, span {6} covers blob 3
        assert got[0, 6 * 2, 6 * 2] > 0.9 and got[0, 6 * 2, 24 * 2] > 0.9 and got[1, 24 * 2, 25 * 2] > 0.9 and got[2, 30, 32] > 0.9


def test_segmentation_cache_gives_the_uncached_masks_and_clusters_once(monkeypatch):
    """sample.py calls get_token_maps twice on the same recorded maps (reference sample.py:78-95); with `cache=` the second call must
    return exactly what an uncached call returns and must not run SpectralClustering again."""
    import sklearn.cluster
    from rich_text_to_image_amd.attention_utils import get_token_maps
    selfm, crossm = synthetic_attention_maps(0)
    toks_a, toks_b = [torch.tensor([2, 3])], [torch.tensor([2, 3]), torch.tensor([6])]
    kw = dict(seed=4, segment_threshold=0.3, num_segments=5, device="cpu")
    ref_a = get_token_maps(selfm, crossm, {}, None, 64, 64, toks_a, **kw)
    ref_b = get_token_maps(selfm, crossm, {}, None, 64, 64, toks_b, **kw)
    calls = []
    real = sklearn.cluster.SpectralClustering

    class Counting(real):
        def fit_predict(self, X, y=None):
            calls.append(1)
            return super().fit_predict(X, y)
    monkeypatch.setattr(sklearn.cluster, "SpectralClustering", Counting)
    cache = {}
    got_a = get_token_maps(selfm, crossm, {}, None, 64, 64, toks_a, cache=cache, **kw)
    got_b = get_token_maps(selfm, crossm, {}, None, 64, 64, toks_b, cache=cache, **kw)
    assert len(calls) == 1
    for g, r in zip(got_a + got_b, ref_a + ref_b):
        assert torch.equal(g, r)
    # another seed / segment count is another key: clustered again
    get_token_maps(selfm, crossm, {}, None, 64, 64, toks_b, cache=cache, seed=5, segment_threshold=0.3, num_segments=5, device="cpu")
    assert len(calls) == 2


def test_single_threaded_clustering_gives_the_default_pools_labels(monkeypatch):
    """get_token_maps runs sklearn's SpectralClustering under threadpool_limits(1) (100 tiny k-means restarts pay the fork / join of a
    256-thread host pool): the masks must be the ones the untouched pools give - and the golden test above already holds the limited
    run against the REFERENCE function's output."""
    from rich_text_to_image_amd.attention_utils import get_token_maps
    selfm, crossm = synthetic_attention_maps(1)
    toks = [torch.tensor([2, 3]), torch.tensor([6])]
    out = {}
    for thr in ("1", "0"):
        monkeypatch.setenv("RTDIFF_CLUSTER_THREADS", thr)
        out[thr] = get_token_maps(selfm, crossm, {}, None, 64, 64, toks, seed=4, segment_threshold=0.3, num_segments=5, device="cpu")
    for a, b in zip(out["1"], out["0"]):
        assert torch.equal(a, b)


def test_same_size_bicubic_antialias_resize_is_the_identity():
    """The port drops the reference's resize of the 32 x 32 self-attention maps to 32 x 32 (attention_utils.py:246-251): it must be
    the identity, bit for bit, in this torch build - including the reference's permute / reshape round trip around it."""
    g = torch.Generator().manual_seed(0)
    m = torch.rand(1, 1024, 1024, generator=g) * torch.logspace(-6, 0, 1024).unsqueeze(0)
    a = m.reshape(1, 32, 32, 1024).permute([3, 0, 1, 2]).float().cpu()
    b = torch.nn.functional.interpolate(a, (32, 32), mode='bicubic', antialias=True)
    assert torch.equal(b.permute([1, 2, 3, 0]).reshape(1, 1024, 1024), m)


def test_layer_lists_match_the_reference_names():
    from rich_text_to_image_amd import attention_utils as au
    from rich_text_to_image_amd.engine import Engine, SD15_CONFIG, SDXL_CONFIG
    for cfg, lists in ((SD15_CONFIG, au.SelfAttentionLayers + au.CrossAttentionLayers), (SDXL_CONFIG, au.CrossAttentionLayers_XL)):
        e = Engine(cfg, 64, 64, device=-1)
        names = {n for n, _, _ in e.attn_modules()}
        assert set(lists) <= names
        e.close()


def test_return_vis_gives_the_reference_triple(tmp_path):
    """get_token_maps(..., return_vis=True) -> (masks, segments_vis, token_maps_vis) (attention_utils.py:271-277,338-339): the same masks
    as the plain call, two uint8 RGB pictures, and the files the reference writes next to them."""
    import numpy as np
    from oracle.synth import synthetic_attention_maps
    from rich_text_to_image_amd.attention_utils import get_token_maps
    selfm, crossm = synthetic_attention_maps(seed=3)
    obj = [torch.tensor([2]), torch.tensor([3, 6])]
    toks = [f"w{i}</w>" for i in range(77)]
    kw = dict(width=64, height=64, obj_tokens=obj, seed=1, tokens_vis=toks, segment_threshold=0.3, num_segments=5, device="cpu")
    plain = get_token_maps(selfm, crossm, None, str(tmp_path), **kw)
    maps, seg_vis, tok_vis = get_token_maps(selfm, crossm, None, str(tmp_path), return_vis=True, **kw)
    assert len(maps) == len(plain) == 3 and all(torch.equal(a, b) for a, b in zip(maps, plain))
    for v in (seg_vis, tok_vis):
        assert isinstance(v, np.ndarray) and v.dtype == np.uint8 and v.ndim == 3 and v.shape[2] == 3 and v.shape[0] > 50
    assert len(np.unique(seg_vis.reshape(-1, 3), axis=0)) >= 5            # five clusters, five colours (+ the white margin)
    assert (tmp_path / "segmentation_k5_seed1.jpg").exists() and (tmp_path / "average_seed1_attn1.png").exists()


def test_maps_of_an_image_with_height_unlike_width_are_refused_with_a_clear_error():
    """The token-map path reads every recorded map as a sqrt(tokens) x sqrt(tokens) grid (attention_utils.py:246, :279 of the reference):
    square images only.  height != width is refused outright, and maps recorded at 256x384 (latent 32x48: 1536 / 384 tokens) are refused
    by name before any reshape - not by an empty torch.cat or a reshape error further down."""
    import pytest
    from rich_text_to_image_amd.attention_utils import get_token_maps
    g = torch.Generator().manual_seed(0)
    selfm = {"down.self": torch.rand(1, 1536, 1536, generator=g)}
    crossm = {"down.cross": torch.rand(1, 1536, 77, generator=g), "mid.cross": torch.rand(1, 384, 77, generator=g)}
    with pytest.raises(ValueError, match="not a square grid"):
        get_token_maps(selfm, crossm, {}, None, 256, 256, [torch.tensor([2, 3])], seed=4, device="cpu")      # (sizes equal: the maps themselves are refused)
    # square maps (a 1:4 image records 4096 / 1024 / 256 tokens: all perfect squares) with height != width: refused by the sizes themselves,
    # with a filled cache as well
    sq, sqc = synthetic_attention_maps(0, n_self=1, n_cross=1)
    cache = {}
    get_token_maps(sq, sqc, {}, None, 64, 64, [torch.tensor([2, 3])], seed=4, device="cpu", cache=cache)
    for kw in ({}, {"cache": cache}):
        with pytest.raises(ValueError, match="height == width"):
            get_token_maps(sq, sqc, {}, None, 256, 64, [torch.tensor([2, 3])], seed=4, device="cpu", **kw)
    # a square self-attention map next to a non-square cross-attention map: refused as well (the cross maps are reshaped too)
    sq, _ = synthetic_attention_maps(0, n_self=1, n_cross=1)
    with pytest.raises(ValueError, match="mid.cross"):
        get_token_maps(sq, {"mid.cross": crossm["mid.cross"]}, {}, None, 64, 64, [torch.tensor([2, 3])], seed=4, device="cpu")
