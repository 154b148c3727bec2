"""CLIP vision encoder on the engine's operators: replaces transformers' `CLIPVisionModelWithProjection` as IP-Adapter calls it
(`image_encoder(pixel_values).image_embeds`, and `.hidden_states[-2]` for the "plus" adapters' Resampler), so that an image prompt can
be a picture instead of a ready embedding.  Mirrors clip_text_encoder.py: every contraction is `rt_op_gemm` (bf16 MFMA, fp32
accumulate) - the patch convolution included, over the patch rows `rt_op_patchify` writes -, LayerNorm is `rt_op_layernorm`, the
class-token / position / pre-LayerNorm front end and the bidirectional attention are the kernels of `csrc/vision.hip`; the residual
stream is fp32.  Weights come under the transformers state-dict names (`vision_model.encoder.layers.N.self_attn.q_proj.weight`, ...).
torch allocates buffers, gathers the class rows and wraps results - no torch arithmetic on the path.

`preprocess` is CLIPImageProcessor's geometry on the host (RGB, bicubic resize of the shortest edge, centre crop) and returns uint8:
rescaling and normalisation happen in `rt_op_patchify`.

Limits: at most 640 tokens per image ((image_size / patch_size)^2 + 1), head dim a multiple of 8 and <= 128, hidden size <= 2048."""
import ctypes as C
import json
import os
import types

import torch

from .engine import RtError, load_library

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
MAX_TOKENS = 640


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _getter(config):
    return (lambda k, d=None: config.get(k, d)) if isinstance(config, dict) else (lambda k, d=None: getattr(config, k, d))


def empty_state_dict(config):
    """Zero tensors under the transformers CLIPVisionModelWithProjection key names with the shapes `config` implies."""
    g = _getter(config)
    Cc, L, I, S, p = g("hidden_size"), g("num_hidden_layers"), g("intermediate_size"), g("image_size", 224), g("patch_size", 14)
    N = (S // p) ** 2 + 1
    z = lambda *s: torch.zeros(*s)
    v = "vision_model."
    sd = {v + "embeddings.class_embedding": z(Cc), v + "embeddings.patch_embedding.weight": z(Cc, g("num_channels", 3), p, p),
          v + "embeddings.position_embedding.weight": z(N, Cc), v + "pre_layrnorm.weight": z(Cc), v + "pre_layrnorm.bias": z(Cc),
          v + "post_layernorm.weight": z(Cc), v + "post_layernorm.bias": z(Cc), "visual_projection.weight": z(g("projection_dim", 512), Cc)}
    for i in range(L):
        q = f"{v}encoder.layers.{i}."
        for n in "qkv":
            sd[q + f"self_attn.{n}_proj.weight"], sd[q + f"self_attn.{n}_proj.bias"] = z(Cc, Cc), z(Cc)
        sd[q + "self_attn.out_proj.weight"], sd[q + "self_attn.out_proj.bias"] = z(Cc, Cc), z(Cc)
        for n in ("layer_norm1", "layer_norm2"):
            sd[q + n + ".weight"], sd[q + n + ".bias"] = z(Cc), z(Cc)
        sd[q + "mlp.fc1.weight"], sd[q + "mlp.fc1.bias"] = z(I, Cc), z(I)
        sd[q + "mlp.fc2.weight"], sd[q + "mlp.fc2.bias"] = z(Cc, I), z(Cc)
    return sd


def check_config(config, who="CLIP vision config"):
    """The shape limits of the kernels as a ValueError naming the key (no GPU needed)."""
    g = _getter(config)
    for k in ("hidden_size", "num_attention_heads", "num_hidden_layers", "intermediate_size"):
        if not isinstance(g(k), int) or g(k) <= 0:
            raise ValueError(f"{who}: {k} must be a positive integer, got {g(k)!r}")
    Cc, H, I, S, p = g("hidden_size"), g("num_attention_heads"), g("intermediate_size"), g("image_size", 224), g("patch_size", 14)
    if g("num_channels", 3) != 3:
        raise ValueError(f"{who}: num_channels must be 3, got {g('num_channels')}")
    if g("hidden_act", "quick_gelu") not in ("quick_gelu", "gelu"):
        raise ValueError(f"{who}: hidden_act must be quick_gelu or gelu, got {g('hidden_act')!r}")
    if Cc % 8 or I % 8 or Cc > 2048:
        raise ValueError(f"{who}: hidden_size / intermediate_size must be multiples of 8 and hidden_size <= 2048, got {Cc} / {I}")
    if Cc % H or (Cc // H) % 8 or Cc // H > 128:
        raise ValueError(f"{who}: hidden_size / num_attention_heads = head dim must be a multiple of 8 and <= 128, got {Cc} / {H}")
    if p <= 0 or S <= 0 or S % p:
        raise ValueError(f"{who}: image_size must be a multiple of patch_size, got {S} / {p}")
    if (S // p) ** 2 + 1 > MAX_TOKENS:
        raise ValueError(f"{who}: image_size {S} at patch_size {p} gives {(S // p) ** 2 + 1} tokens: at most {MAX_TOKENS}")
    if g("projection_dim", 512) % 8:
        raise ValueError(f"{who}: projection_dim must be a multiple of 8, got {g('projection_dim')}")


def check_state_dict(sd, config):
    """Every tensor the encoder reads is there with the shape `config` implies (ValueError naming the key otherwise); returns the key
    prefix ("vision_model." or "" for a bare CLIPVisionTransformer state dict)."""
    p = "vision_model." if any(k.startswith("vision_model.") for k in sd) else ""
    for k, v in empty_state_dict(config).items():
        k = p + k[len("vision_model."):] if k.startswith("vision_model.") else k
        if k not in sd:
            raise ValueError(f"CLIP vision encoder: missing tensor {k}")
        if tuple(sd[k].shape) != tuple(v.shape):
            raise ValueError(f"CLIP vision encoder: {k} has shape {tuple(sd[k].shape)}, the config needs {tuple(v.shape)}")
    return p


class HipCLIPVisionEncoder:
    def __init__(self, state_dict, config, device=0, image_mean=CLIP_MEAN, image_std=CLIP_STD):
        """config: transformers CLIPVisionConfig or a dict with hidden_size, num_attention_heads, num_hidden_layers, intermediate_size,
        hidden_act, layer_norm_eps, image_size, patch_size, projection_dim."""
        check_config(config)
        g = _getter(config)
        self.C, self.H, self.L, self.I = g("hidden_size"), g("num_attention_heads"), g("num_hidden_layers"), g("intermediate_size")
        self.act = {"quick_gelu": 0, "gelu": 1}[g("hidden_act", "quick_gelu")]
        self.eps, self.S, self.p = g("layer_norm_eps", 1e-5), g("image_size", 224), g("patch_size", 14)
        self.projection_dim = g("projection_dim", 512)
        self.hidden_size = self.C                                               # what a plus adapter's Resampler takes (hidden_states[-2])
        self.N =(self.S // self.p) ** 2 + 1
        self.Kp = (3 * self.p * self.p + 7) // 8 * 8
        self.image_mean, self.image_std = tuple(float(x) for x in image_mean), tuple(float(x) for x in image_std)
        if len(self.image_mean) != 3 or len(self.image_std) != 3 or min(self.image_std) <= 0:
            raise ValueError(f"image_mean / image_std must be three numbers each, std > 0, got {image_mean} / {image_std}")
        sd = {k: v.detach() for k, v in state_dict.items()}
        p = check_state_dict(sd, config)
        self.lib = load_library()
        self.device = device
        self.dev = torch.device(f"cuda:{device}")
        f32 = lambda k: sd[k].float().to(self.dev).contiguous()
        b16 = lambda t: t.to(torch.bfloat16).to(self.dev).contiguous()
        self.cls, self.pos = f32(p + "embeddings.class_embedding"), f32(p + "embeddings.position_embedding.weight")
        wp = torch.zeros(self.C, self.Kp)                                       # conv weight [C, 3, p, p] flattened, zero columns up to Kp
        wp[:, :3 * self.p * self.p] = sd[p + "embeddings.patch_embedding.weight"].float().reshape(self.C, -1)
        self.wpatch = b16(wp)
        self.pre = (f32(p + "pre_layrnorm.weight"), f32(p + "pre_layrnorm.bias"))
        self.layers = []
        for i in range(self.L):
            q = f"{p}encoder.layers.{i}."
            wqkv = torch.cat([sd[q + f"self_attn.{n}_proj.weight"].float() for n in "qkv"])
            bqkv = torch.cat([sd[q + f"self_attn.{n}_proj.bias"].float() for n in "qkv"])
            self.layers.append(dict(
                ln1=(f32(q + "layer_norm1.weight"), f32(q + "layer_norm1.bias")), ln2=(f32(q + "layer_norm2.weight"), f32(q + "layer_norm2.bias")),
                wqkv=b16(wqkv), bqkv=bqkv.to(self.dev).contiguous(), wo=b16(sd[q + "self_attn.out_proj.weight"].float()), bo=f32(q + "self_attn.out_proj.bias"),
                w1=b16(sd[q + "mlp.fc1.weight"].float()), b1=f32(q + "mlp.fc1.bias"), w2=b16(sd[q + "mlp.fc2.weight"].float()), b2=f32(q + "mlp.fc2.bias")))
        self.post = (f32(p + "post_layernorm.weight"), f32(p + "post_layernorm.bias"))
        self.wproj = b16(sd["visual_projection.weight"].float())
        self._mean = (C.c_float * 3)(*self.image_mean)
        self._std = (C.c_float * 3)(*self.image_std)
        self.dtype = torch.float32

    def parameter_tensors(self):
        """Every device-resident weight in a fixed order."""
        out = [self.cls, self.pos, self.wpatch, self.pre[0], self.pre[1]]
        for ly in self.layers:
            out += [ly["ln1"][0], ly["ln1"][1], ly["ln2"][0], ly["ln2"][1], ly["wqkv"], ly["bqkv"], ly["wo"], ly["bo"], ly["w1"], ly["b1"],
                    ly["w2"], ly["b2"]]
        out += [self.post[0], self.post[1], self.wproj]
        return out

    def _chk(self, rc):
        if rc != 0:
            raise RtError(rc, self.lib.rt_op_last_error().decode())

    def _gemm(self, A, W, bias, out, epi=0, res=None):
        M, K = A.shape
        N = W.shape[0]
        self._chk(self.lib.rt_op_gemm(_ptr(A), _ptr(W), _ptr(bias), _ptr(out), _ptr(res), None, 0, epi, M, N, K, A.stride(0), W.stride(0),
                                      out.stride(0), res.stride(0) if res is not None else 0, 0, 0, 0, 0, 0, 0, 0, None))

    def _ln(self, x, wb):
        out = torch.empty(x.shape, device=self.dev, dtype=torch.bfloat16)
        self._chk(self.lib.rt_op_layernorm(_ptr(x), _ptr(wb[0]), _ptr(wb[1]), _ptr(out), x.shape[0], x.shape[1], C.c_float(self.eps), None))
        return out

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def __call__(self, pixels_u8, output_hidden_states=False, **_):
        px = torch.as_tensor(pixels_u8)
        if px.dtype != torch.uint8 or px.dim() != 4 or tuple(px.shape[1:]) != (self.S, self.S, 3):
            raise ValueError(f"pixels must be uint8 [B, {self.S}, {self.S}, 3] (preprocess), got {px.dtype} {tuple(px.shape)}")
        px = px.to(self.dev).contiguous()
        B, N, Cc, H = px.shape[0], self.N, self.C, self.H
        M, d = B * N, Cc // H
        with torch.cuda.device(self.dev):
            rows = torch.empty(B * (N - 1), self.Kp, device=self.dev, dtype=torch.bfloat16)
            self._chk(self.lib.rt_op_patchify(_ptr(px), _ptr(rows), B, self.S, self.p, self.Kp, self._mean, self._std, None))
            patch = torch.empty(B * (N - 1), Cc, device=self.dev)
            self._gemm(rows, self.wpatch, None, patch, epi=1)                       # the patch convolution (no bias)
            x = torch.empty(M, Cc, device=self.dev)
            self._chk(self.lib.rt_op_vit_embed(_ptr(patch), Cc, _ptr(self.cls), _ptr(self.pos), _ptr(self.pre[0]), _ptr(self.pre[1]), _ptr(x),
                                               B, N, Cc, C.c_float(self.eps), None))
            hidden = [x.reshape(B, N, Cc).clone()] if output_hidden_states else None
            qkv = torch.empty(M, 3 * Cc, device=self.dev, dtype=torch.bfloat16)
            att = torch.empty(M, Cc, device=self.dev, dtype=torch.bfloat16)
            f1 = torch.empty(M, self.I, device=self.dev, dtype=torch.bfloat16)
            f2 = torch.empty_like(f1)
            for ly in self.layers:
                h = self._ln(x, ly["ln1"])
                self._gemm(h, ly["wqkv"], ly["bqkv"], qkv)
                self._chk(self.lib.rt_op_bidir_attention(_ptr(qkv), C.c_void_p(qkv.data_ptr() + 2 * Cc), C.c_void_p(qkv.data_ptr() + 4 * Cc), 3 * Cc,
                                                         _ptr(att), Cc, B, H, N, d, C.c_float(d ** -0.5), None))
                self._gemm(att, ly["wo"], ly["bo"], x, epi=1, res=x)
                h = self._ln(x, ly["ln2"])
                self._gemm(h, ly["w1"], ly["b1"], f1)
                self._chk(self.lib.rt_op_activation(_ptr(f1), _ptr(f2), f1.numel(), self.act, None))
                self._gemm(f2, ly["w2"], ly["b2"], x, epi=1, res=x)
                if output_hidden_states:
                    hidden.append(x.reshape(B, N, Cc).clone())
            last = x.reshape(B, N, Cc).clone()                                      # transformers: the encoder output, NOT post-LayerNorm'd
            cls_rows = last[:, 0].contiguous()                                      # gather only
            pooled = self._ln(cls_rows, self.post)                                  # bf16 [B, C]
            emb = torch.empty(B, self.projection_dim, device=self.dev)
            self._gemm(pooled, self.wproj, None, emb, epi=1)
            torch.cuda.synchronize(self.dev)
        return types.SimpleNamespace(image_embeds=emb, last_hidden_state=last, pooler_output=pooled.float(),
                                     hidden_states=tuple(hidden) if hidden else None)


# ---------------------------------------------------------------------------------------------------------------- host side
def preprocess(image, size=224):
    """CLIPImageProcessor's geometry: RGB, bicubic resize of the shortest edge to `size` (the long edge keeps the aspect ratio,
    truncated), centre crop to size x size -> uint8 [size, size, 3] (numpy).  `image`: a path, a PIL image or an [H, W, 3] uint8 array."""
    import numpy as np
    from PIL import Image
    if isinstance(image, (str, os.PathLike)):
        if not os.path.isfile(image):
            raise ValueError(f"image file not found: {image}")
        try:
            img = Image.open(image)
            img.load()
        except Exception as e:
            raise ValueError(f"{image}: not a readable image ({e})")
    elif isinstance(image, Image.Image):
        img = image
    else:
        arr = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3 or arr.shape[0] < 1 or arr.shape[1] < 1:
            raise ValueError(f"image must be a path, a PIL image or an [H, W, 3] uint8 array, got {arr.dtype} {arr.shape}")
        img = Image.fromarray(np.ascontiguousarray(arr))
    img = img.convert("RGB")
    w, h = img.size
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = int(size), int(size * long / short)
    nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
    img = img.resize((nw, nh), resample=Image.BICUBIC)
    top, left = (nh - size) // 2, (nw - size) // 2
    return np.asarray(img.crop((left, top, left + size, top + size)), dtype=np.uint8)


def read_image_encoder(path):
    """A directory in the Hugging Face layout - config.json, model.safetensors or pytorch_model.bin, optionally preprocessor_config.json
    (what IP-Adapter ships as models/image_encoder/) -> (state_dict, config dict, image_mean, image_std, size).  ValueError naming the
    file or key otherwise.  No GPU needed."""
    path = os.fspath(path)
    cfg_file = os.path.join(path, "config.json")
    if not os.path.isdir(path):
        raise ValueError(f"image encoder: {path} is not a directory (expected config.json + model.safetensors / pytorch_model.bin)")
    if not os.path.isfile(cfg_file):
        raise ValueError(f"image encoder: {cfg_file} not found")
    with open(cfg_file) as f:
        cfg = json.load(f)
    if isinstance(cfg.get("vision_config"), dict) and "hidden_size" not in cfg:      # a full CLIPConfig: its vision half
        cfg = dict(cfg["vision_config"], projection_dim=cfg.get("projection_dim", cfg["vision_config"].get("projection_dim", 512)))
    if cfg.get("model_type") not in (None, "clip_vision_model") or "patch_size" not in cfg or "image_size" not in cfg or "vocab_size" in cfg:
        raise ValueError(f"image encoder: {cfg_file} is not a CLIP vision config (model_type {cfg.get('model_type')!r}; needs image_size and patch_size)")
    check_config(cfg, cfg_file)
    st, pt = os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")
    if os.path.isfile(st):
        from safetensors.torch import load_file
        sd = load_file(st)
    elif os.path.isfile(pt):
        sd = torch.load(pt, map_location="cpu", weights_only=True)
    else:
        raise ValueError(f"image encoder: neither {st} nor {pt} found")
    mean, std, size = CLIP_MEAN, CLIP_STD, cfg["image_size"]
    pp = os.path.join(path, "preprocessor_config.json")
    if os.path.isfile(pp):
        with open(pp) as f:
            pc = json.load(f)
        mean, std = tuple(pc.get("image_mean", mean)), tuple(pc.get("image_std", std))
        cs = pc.get("crop_size", size)
        cs = cs.get("height", size) if isinstance(cs, dict) else cs
        if cs != size:
            raise ValueError(f"image encoder: {pp}: crop_size {cs} differs from the config's image_size {size}")
    try:
        check_state_dict(sd, cfg)
    except ValueError as e:
        raise ValueError(f"image encoder: {st if os.path.isfile(st) else pt}: {e}")
    return sd, cfg, mean, std, size


def load_image_encoder(path, device=0):
    """read_image_encoder + HipCLIPVisionEncoder on `device`."""
    sd, cfg, mean, std, _ = read_image_encoder(path)
    return HipCLIPVisionEncoder(sd, cfg, device=device, image_mean=mean, image_std=std)


class LazyImageEncoder:
    """An encoder directory that has been read and checked on the host; the device object is built on first use, on the device that
    uses it (a pipeline's ranks each load their own, like the VAE encoder)."""
    def __init__(self, path):
        self.path = os.fspath(path)
        self._host = read_image_encoder(self.path)
        cfg = self._host[1]
        self.S, self.projection_dim, self.hidden_size = cfg["image_size"], cfg.get("projection_dim", 512), cfg["hidden_size"]
        self._enc = {}

    def on(self, device):
        if device not in self._enc:
            sd, cfg, mean, std, _ = self._host if self._host is not None else read_image_encoder(self.path)
            self._enc[device] = HipCLIPVisionEncoder(sd, cfg, device=device, image_mean=mean, image_std=std)
            self._host = None                                                       # the host copy of the weights is not kept
        return self._enc[device]
