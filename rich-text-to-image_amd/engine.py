"""ctypes binding of librtdiff.so (include/rtdiff.h).  PyTorch is used for device memory only."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "librtdiff.so")
_lib = None

RT_MAX_LEVELS = 4
RT_MAX_STREAMS = 16
DTYPE_F32, DTYPE_F16, DTYPE_BF16 = 0, 1, 2
SCHED_EULER, SCHED_PNDM = 0, 1
PRED_EPSILON, PRED_V = 0, 1
PREDICTION_TYPES = {"epsilon": PRED_EPSILON, "v_prediction": PRED_V}
A_DENSE, A_CONV3, A_CONV3_S2, A_CONV3_UP2, A_CONV3_S2P0 = 0, 1, 2, 3, 4
EPI_BF16, EPI_F32, EPI_BF16_TEMB, EPI_GEGLU, EPI_F16 = 0, 1, 2, 3, 4

# UNet architectures of the two pipelines (models/region_diffusion.py:32, region_diffusion_sdxl.py:115;
# values = the published unet/config.json of runwayml/stable-diffusion-v1-5 and
# stabilityai/stable-diffusion-xl-base-1.0, validated by parameter count in SURVEY.md section 8)
SD15_CONFIG = dict(
    in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280, 1280),
    down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
    up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
    layers_per_block=2, transformer_layers_per_block=1, attention_head_dim=8, cross_attention_dim=768,
    norm_num_groups=32, norm_eps=1e-5, use_linear_projection=False, addition_embed_type=None,
    addition_time_embed_dim=None, projection_class_embeddings_input_dim=None)
SDXL_CONFIG = dict(
    in_channels=4, out_channels=4, block_out_channels=(320, 640, 1280),
    down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
    up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"),
    layers_per_block=2, transformer_layers_per_block=(1, 2, 10), attention_head_dim=(5, 10, 20),
    cross_attention_dim=2048, norm_num_groups=32, norm_eps=1e-5, use_linear_projection=True,
    addition_embed_type="text_time", addition_time_embed_dim=256, projection_class_embeddings_input_dim=2816)


class RtConfig(C.Structure):
    _fields_ = [
        ("n_levels", C.c_int),
        ("block_out_channels", C.c_int * RT_MAX_LEVELS),
        ("down_has_attn", C.c_int * RT_MAX_LEVELS),
        ("up_has_attn", C.c_int * RT_MAX_LEVELS),
        ("layers_per_block", C.c_int * RT_MAX_LEVELS),
        ("transformer_layers", C.c_int * RT_MAX_LEVELS),
        ("heads", C.c_int * RT_MAX_LEVELS),
        ("cross_attention_dim", C.c_int),
        ("norm_groups", C.c_int),
        ("norm_eps", C.c_float),
        ("use_linear_projection", C.c_int),
        ("addition_text_time", C.c_int),
        ("addition_time_embed_dim", C.c_int),
        ("projection_class_embeddings_input_dim", C.c_int),
        ("in_channels", C.c_int), ("out_channels", C.c_int),
        ("latent_h", C.c_int), ("latent_w", C.c_int),
        ("max_streams", C.c_int), ("max_prompts", C.c_int),
        ("max_keys", C.c_int),
        ("ip_tokens", C.c_int),
        ("controlnet", C.c_int),
        ("control_hint_channels", C.c_int),
        ("control_embed_channels", C.c_int * 4),
        ("lora_rank", C.c_int),
        ("lora_targets", C.c_int),
    ]


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"librtdiff error {code}: {msg}")
        self.code = code


_SYMBOLS = [
    "rt_create", "rt_destroy", "rt_last_error", "rt_set_stream", "rt_synchronize", "rt_weight_count",
    "rt_weight_info", "rt_bind_weight", "rt_weights_missing", "rt_arena_info", "rt_arena_mark_bound",
    "rt_set_prompts", "rt_set_masks", "rt_set_fontsize", "rt_set_schedule", "rt_set_latents", "rt_get_latents",
    "rt_region_step", "rt_plain_step", "rt_unet_forward", "rt_op_gemm", "rt_op_attention", "rt_op_groupnorm",
    "rt_op_layernorm", "rt_op_layernorm_f16", "rt_op_small_linear", "rt_op_timestep_embed", "rt_op_last_error", "rt_profile_enable",
    "rt_profile_read", "rt_op_gemm_force_config", "rt_op_gemm_debug", "rt_attn_store_enable", "rt_attn_store_reset",
    "rt_attn_store_read", "rt_attn_module_count", "rt_attn_module_info", "rt_get_state_ptrs", "rt_background_blend", "rt_vae_create", "rt_vae_destroy",
    "rt_vae_last_error", "rt_vae_weight_count", "rt_vae_weight_info", "rt_vae_bind_weight", "rt_vae_synchronize", "rt_vae_decode",
    "rt_vae_color_guidance", "rt_vae_arena_info", "rt_vae_arena_mark_bound", "rt_op_cast_bf16", "rt_op_attention_probs_avg", "rt_op_embed", "rt_op_activation", "rt_op_causal_attention",
    "rt_op_cross_attn_block", "rt_op_gemm16_variant", "rt_op_gemm16_pick", "rt_op_split_plan", "rt_profile_read2", "rt_op_gemm_qk_vt", "rt_op_gemm_pair_pick",
    "rt_region_step_part", "rt_region_step_finish", "rt_eps_info", "rt_op_split_range",
    "rt_op_ln_gemm", "rt_op_gemm_emit_partials", "rt_op_ln_partials", "rt_op_probes_built", "rt_op_attention_units_plan",
    "rt_plain_step_part", "rt_plain_step_finish", "rt_vae_encoder_create", "rt_vae_encode", "rt_vae_posterior_sample",
    "rt_set_source", "rt_noise_latents", "rt_source_blend",
    "rt_op_gemm_debug2", "rt_op_pack_upconv", "rt_op_upconv",
    "rt_set_prompts_keys", "rt_op_attention_keys",
    "rt_set_noise_seed", "rt_op_step_noise",
    "rt_set_prediction", "rt_op_guided_prediction",
    "rt_op_attention_store_handover",
    "rt_op_gemm_route", "rt_op_groupnorm_form", "rt_op_cross_route",
    "rt_set_freeu", "rt_op_freeu",
    "rt_op_gemm_hilo", "rt_op_gemm_hilo_route", "rt_op_split_bf16", "rt_op_vae_groupnorm_nchunk", "rt_op_vae_groupnorm", "rt_op_vae_groupnorm_bwd",
    "rt_op_softmax_rows", "rt_op_softmax_bwd", "rt_op_transpose_bf16", "rt_op_sumpool2x2", "rt_op_pq_conv_fwd", "rt_op_pq_conv_bwd_update",
    "rt_op_color_loss_grad",
    "rt_set_image_prompts", "rt_op_ip_attention",
    "rt_unet_forward_trace", "rt_trace_module_count", "rt_trace_module_info",
    "rt_op_patchify", "rt_op_vit_embed", "rt_op_bidir_attention",
    "rt_op_latent_attention",
    "rt_set_control_hint", "rt_control_embedding_read", "rt_set_control_scales", "rt_op_control_add",
    "rt_op_lora_add", "rt_set_lora_columns", "rt_set_lora_scales", "rt_attn_cache_info", "rt_op_lora_geglu",
    "rt_set_pag_layers", "rt_set_pag_scales", "rt_plain_streams", "rt_unet_forward_perturbed", "rt_op_identity_attention", "rt_op_pag_fold",
]


def load_library(path=None):
    """Loads librtdiff.so; fails loudly when the HIP extension has not been built (no CPU fallback)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("RTDIFF_LIB_PATH") or _LIB_PATH          # RTDIFF_LIB_PATH: A/B builds of the same ABI (benchmarks only)
    if not os.path.exists(p):
        raise RtError(-3, f"{p} not found: build it with `python __graft_entry__.py build` "
                          "(hipcc --offload-arch=gfx950); there is no fallback path")
    lib = C.CDLL(p)
    # RTDIFF_ALLOW_MISSING_SYMBOLS: A/B runs against an OLDER build of the library (benchmarks / regression hunts only)
    names = [s for s in _SYMBOLS if hasattr(lib, s)] if os.environ.get("RTDIFF_ALLOW_MISSING_SYMBOLS") else _SYMBOLS
    for s in names:
        getattr(lib, s)          # AttributeError if a declared symbol is missing
    lib.rt_last_error.restype = C.c_char_p
    lib.rt_op_last_error.restype = C.c_char_p
    lib.rt_last_error.argtypes = [C.c_void_p]
    lib.rt_vae_last_error.restype = C.c_char_p
    lib.rt_vae_last_error.argtypes = [C.c_void_p]
    for name in names:
        if name not in ("rt_last_error", "rt_op_last_error", "rt_vae_last_error"):
            getattr(lib, name).restype = C.c_int
    flags = int(os.environ.get("RTDIFF_DEBUG_FLAGS", "0"))      # A/B switches of rt_op_gemm_debug (benchmarks only)
    if flags:
        lib.rt_op_gemm_debug(flags)
    flags2 = int(os.environ.get("RTDIFF_DEBUG_FLAGS2", "0"))    # ... and of rt_op_gemm_debug2
    if flags2 and hasattr(lib, "rt_op_gemm_debug2"):
        lib.rt_op_gemm_debug2(flags2)
    if path is None:
        _lib = lib
    return lib


def _tup(v, n):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * n


CONTROL_EMBED_CHANNELS = (16, 32, 96, 256)      # diffusers' ControlNetModel default `conditioning_embedding_out_channels`


def config_from_dict(cfg, latent_h, latent_w, max_streams=8, max_prompts=8, max_keys=77, ip_tokens=0, controlnet=None, lora_rank=0,
                     lora_targets=0):
    """UNet2DConditionModel kwargs (reference config.json) -> rt_config.  max_keys: keys of the longest prompt (77 per CLIP window).
    lora_rank: rank columns of the regional LoRA adapters (a multiple of 16 up to 128); 0 = none: the weight table is the reference's.
    lora_targets: 0 = the adapters sit on the eight attention projections; 1 = on ff.net.0.proj, ff.net.2, proj_in and proj_out as well.
    ip_tokens: image tokens per prompt slot of an IP-Adapter (1 .. 16); 0 = none: the weight table is the reference's state_dict layout.
    controlnet: None = no ControlNet (likewise), or dict(embed_channels=(16, 32, 96, 256), hint_channels=3) - either key optional."""
    c = RtConfig()
    boc = tuple(cfg["block_out_channels"])
    n = len(boc)
    c.n_levels = n
    lpb, tl, heads = _tup(cfg["layers_per_block"], n), _tup(cfg["transformer_layers_per_block"], n), _tup(cfg["attention_head_dim"], n)
    for i in range(n):
        c.block_out_channels[i] = boc[i]
        c.down_has_attn[i] = int(cfg["down_block_types"][i] == "CrossAttnDownBlock2D")
        c.up_has_attn[i] = int(cfg["up_block_types"][i] == "CrossAttnUpBlock2D")
        c.layers_per_block[i] = lpb[i]
        c.transformer_layers[i] = tl[i]
        c.heads[i] = heads[i]
        if cfg["down_block_types"][i] not in ("CrossAttnDownBlock2D", "DownBlock2D") or \
           cfg["up_block_types"][i] not in ("CrossAttnUpBlock2D", "UpBlock2D"):
            raise ValueError("unsupported block type (only the SD / SDXL block types are on the hot path)")
    c.cross_attention_dim = cfg["cross_attention_dim"]
    c.norm_groups = cfg["norm_num_groups"]
    c.norm_eps = cfg.get("norm_eps", 1e-5)
    c.use_linear_projection = int(bool(cfg["use_linear_projection"]))
    c.addition_text_time = int(cfg.get("addition_embed_type") == "text_time")
    c.addition_time_embed_dim = cfg.get("addition_time_embed_dim") or 0
    c.projection_class_embeddings_input_dim = cfg.get("projection_class_embeddings_input_dim") or 0
    c.in_channels, c.out_channels = cfg["in_channels"], cfg["out_channels"]
    c.latent_h, c.latent_w = latent_h, latent_w
    c.max_streams, c.max_prompts = max_streams, max_prompts
    c.max_keys = max_keys
    c.ip_tokens = int(ip_tokens)
    c.lora_rank = int(lora_rank)
    c.lora_targets = int(lora_targets)
    if controlnet is not None:
        unknown = set(controlnet) - {"embed_channels", "hint_channels"}
        if unknown:
            raise ValueError(f"controlnet: unknown keys {sorted(unknown)}")
        ch = tuple(int(v) for v in (controlnet.get("embed_channels") or CONTROL_EMBED_CHANNELS))
        if len(ch) != 4 or any(v < 8 or v % 8 for v in ch):
            raise ValueError(f"controlnet: embed_channels must be four multiples of 8, got {ch}")
        c.controlnet = 1
        c.control_hint_channels = int(controlnet.get("hint_channels") or 3)
        for i, v in enumerate(ch):
            c.control_embed_channels[i] = v
    return c


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Engine:
    """One engine = one GPU.  Mirrors the C ABI one to one; see include/rtdiff.h for semantics."""

    def __init__(self, cfg_dict, latent_h, latent_w, device=0, max_streams=8, max_prompts=8, max_keys=77, ip_tokens=0, controlnet=None,
                 lora_rank=0, lora_targets=0):
        self.lib = load_library()
        self.cfg_dict = dict(cfg_dict)
        self.cfg = config_from_dict(cfg_dict, latent_h, latent_w, max_streams, max_prompts, max_keys, ip_tokens, controlnet, lora_rank, lora_targets)
        self.lora_rank, self.lora_targets = int(lora_rank), int(lora_targets)
        self.controlnet = dict(controlnet) if controlnet is not None else None
        self.max_keys = max_keys
        self.ip_tokens = int(ip_tokens)
        self.h = C.c_void_p()
        self.device = device
        rc = self.lib.rt_create(C.byref(self.cfg), C.c_int(device), C.byref(self.h))
        if rc != 0:
            raise RtError(rc, self.lib.rt_last_error(None).decode())
        self._keep = []

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.rt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise RtError(rc, self.lib.rt_last_error(self.h).decode())

    # ---- weights
    def weight_table(self):
        n = self.lib.rt_weight_count(self.h)
        out = []
        name = C.create_string_buffer(256)
        shape = (C.c_int64 * 4)()
        nd = C.c_int()
        for i in range(n):
            self._chk(self.lib.rt_weight_info(self.h, i, name, 256, shape, C.byref(nd)))
            out.append((name.value.decode(), tuple(shape[k] for k in range(nd.value))))
        return out

    def bind_weight(self, name, t):
        import torch
        dt = {torch.float32: DTYPE_F32, torch.float16: DTYPE_F16, torch.bfloat16: DTYPE_BF16}[t.dtype]
        t = t.contiguous()
        shape = (C.c_int64 * max(1, t.dim()))(*t.shape)
        self._chk(self.lib.rt_bind_weight(self.h, name.encode(), _ptr(t), dt, shape, t.dim()))

    def load_state_dict(self, sd, device=None):
        """Packs a reference-layout state_dict (CPU or GPU tensors) into the engine's bf16 arena."""
        import torch
        dev = device or f"cuda:{self.device}"
        for name, shape in self.weight_table():
            if name not in sd and name.startswith("lora."):          # no regional adapter resident (bind_regional_loras fills these): zero factors
                self.bind_weight(name, torch.zeros(shape, device=dev))
                continue
            if name not in sd:
                raise RtError(-4, f"missing weight {name}")
            t = sd[name].to(dev, non_blocking=False)
            self.bind_weight(name, t)
        self.synchronize()

    def init_random_weights(self, seed=0, std_scale=1.0):
        """Random-init weights of the true architecture directly on the GPU (bench / smoke: no checkpoints offline)."""
        import math
        import torch
        dev = f"cuda:{self.device}"
        g = torch.Generator(device=dev).manual_seed(seed)
        for name, shape in self.weight_table():
            if name.endswith(".weight") and len(shape) >= 2:
                fan_in = 1
                for s in shape[1:]:
                    fan_in *= s
                t = (torch.rand(shape, generator=g, device=dev) * 2 - 1) * (std_scale / math.sqrt(fan_in))
            elif name.endswith(".weight"):
                t = 1.0 + 0.1 * (torch.rand(shape, generator=g, device=dev) * 2 - 1)
            else:
                t = 0.05 * (torch.rand(shape, generator=g, device=dev) * 2 - 1)
            self.bind_weight(name, t)
            self.synchronize()
            del t

    def weights_missing(self):
        buf = C.create_string_buffer(1 << 16)
        n = self.lib.rt_weights_missing(self.h, buf, len(buf))
        return n, [s for s in buf.value.decode().split(";") if s]

    def arena(self):
        p, b = C.c_void_p(), C.c_uint64()
        self._chk(self.lib.rt_arena_info(self.h, C.byref(p), C.byref(b)))
        return p.value, b.value

    def arena_mark_bound(self):
        self._chk(self.lib.rt_arena_mark_bound(self.h))

    def synchronize(self):
        self._chk(self.lib.rt_synchronize(self.h))

    def set_stream(self, stream_ptr):
        self._chk(self.lib.rt_set_stream(self.h, C.c_void_p(stream_ptr)))

    # ---- per image
    def set_prompts(self, prompt_embeds, pooled=None, time_ids=None, key_counts=None):
        """prompt_embeds [P, 77 c, D].  key_counts (one per prompt, multiples of 77; default: every row of every prompt is a key): the
        first key_counts[p] rows of prompt p are its keys and the rest is ignored, so prompts of different lengths share one call."""
        import torch
        pe = prompt_embeds.contiguous().float()
        assert pe.dim() == 3 and pe.shape[1] >= 77 and pe.shape[1] % 77 == 0, tuple(pe.shape)
        pl = pooled.contiguous().float() if pooled is not None else None
        tid = (C.c_float * 6)(*[float(v) for v in time_ids.flatten().tolist()[:6]]) if time_ids is not None else None
        if key_counts is None and pe.shape[1] == 77:
            self._chk(self.lib.rt_set_prompts(self.h, _ptr(pe), _ptr(pl), tid, pe.shape[0], pl.shape[1] if pl is not None else 0))
            return
        kc = [int(v) for v in key_counts] if key_counts is not None else [pe.shape[1]] * pe.shape[0]
        assert len(kc) == pe.shape[0], (len(kc), pe.shape[0])
        self._chk(self.lib.rt_set_prompts_keys(self.h, _ptr(pe), (C.c_int * len(kc))(*kc), pe.shape[1], _ptr(pl), tid, pe.shape[0],
                                               pl.shape[1] if pl is not None else 0))

    def set_image_prompts(self, tokens, scales, counts=None):
        """Image prompts of the prompt slots of the last set_prompts (include/rtdiff.h: rt_set_image_prompts; engines built with
        ip_tokens > 0).  tokens [P, ip_tokens, D]: the projected image tokens of slot p (None when every scale is 0); scales [P], 0 = that
        prompt has no image; counts [P] in 1 .. ip_tokens (default: all).  set_prompts switches every image off again."""
        sc = [float(v) for v in scales]
        P = len(sc)
        tk = None
        if tokens is not None:
            tk = tokens.contiguous().float()
            if tk.dim() != 3 or tuple(tk.shape[:2]) != (P, self.ip_tokens) or tk.shape[2] != self.cfg.cross_attention_dim:
                raise ValueError(f"set_image_prompts: tokens must be [{P}, {self.ip_tokens}, {self.cfg.cross_attention_dim}], got {tuple(tk.shape)}")
        cn = None
        if counts is not None:
            cn = [int(v) for v in counts]
            if len(cn) != P:
                raise ValueError(f"set_image_prompts: {len(cn)} counts for {P} scales")
        self._chk(self.lib.rt_set_image_prompts(self.h, _ptr(tk), (C.c_int * P)(*cn) if cn is not None else None, (C.c_float * max(1, P))(*sc), P))

    # ---- ControlNet (include/rtdiff.h: rt_set_control_hint / rt_set_control_scales; engines built with controlnet=dict(...))
    def set_control_hint(self, hint):
        """hint [hint_channels, 8 h, 8 w] (or [1, ...]) fp32, values as the checkpoint expects (usually 0 .. 1): runs the hint embedder once
        and caches the [h w, C0] embedding every controlled stream adds to controlnet.conv_in(x).  None clears the hint.  The hint
        survives set_prompts; a forward at another latent size while a stream is controlled raises."""
        if hint is None:
            self._chk(self.lib.rt_set_control_hint(self.h, None, 0, 0))
            return
        t = hint.to(f"cuda:{self.device}").float().contiguous()
        if t.dim() == 4 and t.shape[0] == 1:
            t = t[0]
        ch = self.cfg.control_hint_channels or 3
        if t.dim() != 3 or t.shape[0] != ch or t.shape[1] % 8 or t.shape[2] % 8:
            raise RtError(-1, f"set_control_hint: the hint must be [{ch}, 8 h, 8 w], got {tuple(hint.shape)}")
        self._chk(self.lib.rt_set_control_hint(self.h, _ptr(t), t.shape[1] // 8, t.shape[2] // 8))

    def set_control_scales(self, scales):
        """One finite scale per prompt slot of the last set_prompts; 0 = a stream that runs that prompt is not controlled (it launches
        nothing new and keeps its bits).  set_prompts resets every scale to 0."""
        sc = [float(v) for v in scales]
        self._chk(self.lib.rt_set_control_scales(self.h, (C.c_float * max(1, len(sc)))(*sc), len(sc)))

    # ---- perturbed-attention guidance (include/rtdiff.h: rt_set_pag_layers / rt_set_pag_scales)
    def set_pag_layers(self, names):
        """The applied attn1 modules, full names as attn_modules() lists them (pag.resolve_layers turns specs such as "mid" into names).
        Survives set_prompts."""
        self._chk(self.lib.rt_set_pag_layers(self.h, ";".join(names).encode()))

    def set_pag_scales(self, scales):
        """One finite sigma per prompt slot of the last set_prompts (slot 0, the negative prompt, must be 0); a slot with sigma != 0 gets a
        perturbed twin stream in every step.  set_prompts resets every sigma to 0."""
        sc = [float(v) for v in scales]
        self._chk(self.lib.rt_set_pag_scales(self.h, (C.c_float * max(1, len(sc)))(*sc) if sc else None, len(sc)))

    PROF_PAG = 10           # pag.hip (identity attention of the twins, the fold of a step): priced in algorithmic HBM bytes

    def profile_read_pag(self):
        n, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
        self._chk(self.lib.rt_profile_read2(self.h, self.PROF_PAG, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)))
        return dict(launches=n.value, total_ms=ms.value, total_flops=fl.value, total_bytes=by.value)

    # ---- regional LoRA (include/rtdiff.h: rt_set_lora_columns / rt_set_lora_scales; engines built with lora_rank > 0)
    def bind_regional_loras(self, adapters):
        """adapters: {name: modules} of regional_lora.parse_adapter, in load order (an empty dict: zero factors everywhere).  Binds the
        lora.* slots of every adapted projection - the concatenation along the rank of regional_lora.concat_module, which the engine
        packs like the base weight beside it - and the column -> adapter map.  Returns the adapter names in column order."""
        import torch
        from . import regional_lora as RL
        dev = f"cuda:{self.device}"
        R = self.lora_rank
        if R <= 0:
            raise RtError(-1, "bind_regional_loras: the engine was built without regional LoRA (lora_rank=0)")
        layout = None
        if adapters:
            layout = RL.rank_layout(adapters)
            if layout[3] > R:
                raise ValueError(f"the adapters' padded ranks {dict(zip(layout[0], layout[1]))} add up to {layout[3]} rank columns; this engine was built for {R}")
        col = [0] * R
        table = dict(self.weight_table())
        # an adapter must run whole: a module this engine has no slot for (ff / proj_in / proj_out on an engine built with lora_targets=0) is refused
        absent = sorted({p for m in (adapters or {}).values() for p in m if f"lora.{p}.down.weight" not in table})
        if absent:
            raise ValueError(f"bind_regional_loras: this engine (lora_targets={self.lora_targets}) has no slots for the adapted modules {absent}; "
                             "build it with lora_targets=1, or parse the adapters with attention_only=True")
        for name, shape in table.items():
            if not name.startswith("lora.") or not name.endswith(".down.weight"):
                continue
            mod = name[len("lora."):-len(".down.weight")]
            K, N = shape[1], table[f"lora.{mod}.up.weight"][0]
            down, up, aor = torch.zeros(R, K), torch.zeros(N, R), torch.zeros(R)
            if adapters:
                d, u, a, c = RL.concat_module(adapters, mod, K, N, layout)
                down[:d.shape[0]], up[:, :u.shape[1]], aor[:a.shape[0]] = d, u, a
                col[:c.shape[0]] = [int(v) for v in c]
            self.bind_weight(f"lora.{mod}.down.weight", down.to(dev))
            self.bind_weight(f"lora.{mod}.up.weight", up.to(dev))
            self.bind_weight(f"lora.{mod}.alpha_over_rank", aor.to(dev))
        self.synchronize()
        self._chk(self.lib.rt_set_lora_columns(self.h, (C.c_int * R)(*col), R))
        return list(layout[0]) if layout else []

    def set_lora_scales(self, scales):
        """scales [P][<= 4]: per prompt slot of the last set_prompts, one finite scale per resident adapter (0 = a stream that runs that
        prompt is not adapted: it is in no new launch and keeps its bits).  set_prompts resets every scale to 0."""
        rows = [[float(s[l]) if l < len(s) else 0.0 for l in range(4)] for s in scales]
        flat = [v for r in rows for v in r]
        self._chk(self.lib.rt_set_lora_scales(self.h, (C.c_float * max(1, len(flat)))(*flat), len(rows)))

    def attn_caches(self):
        """Test seam (rt_attn_cache_info): the attn2 K / V^T caches of every transformer block of the main UNet, in execution order, as
        a list of (kcache, vtcache) int16 views of the engine's own memory (bf16 bits)."""
        import torch
        from .launcher import _DevicePointer
        out = []
        for i in range(self.lib.rt_attn_module_count(self.h) // 2):
            k, v, n = C.c_void_p(), C.c_void_p(), C.c_longlong()
            self._chk(self.lib.rt_attn_cache_info(self.h, i, C.byref(k), C.byref(v), C.byref(n)))
            out.append(tuple(torch.as_tensor(_DevicePointer(p.value, n.value), device=f"cuda:{self.device}").view(torch.int16) for p in (k, v)))
        return out

    def control_embedding(self):
        """The cached hint embedding as fp32 [h w, C0] on the GPU, or None when no hint is set (test seam)."""
        import torch
        r, c = C.c_int(), C.c_int()
        self._chk(self.lib.rt_control_embedding_read(self.h, None, C.byref(r), C.byref(c)))
        if r.value == 0:
            return None
        out = torch.empty(r.value, c.value, device=f"cuda:{self.device}")
        self._chk(self.lib.rt_control_embedding_read(self.h, _ptr(out), C.byref(r), C.byref(c)))
        return out

    PROF_CONTROL = 8        # control_add_kernel (the ControlNet residual adds of a step): priced in algorithmic HBM bytes

    def profile_read_control(self):
        n, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
        self._chk(self.lib.rt_profile_read2(self.h, self.PROF_CONTROL, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)))
        return dict(launches=n.value, total_ms=ms.value, total_flops=fl.value, total_bytes=by.value)

    def set_masks(self, masks):
        """masks: list of [1,4,h,w] tensors (model.masks) or one [R,4,h,w] tensor."""
        import torch
        m = torch.cat(list(masks), 0) if isinstance(masks, (list, tuple)) else masks
        m = m.contiguous().float()
        self._chk(self.lib.rt_set_masks(self.h, _ptr(m), m.shape[0], m.shape[2], m.shape[3]))
        self.synchronize()

    def set_fontsize(self, word_pos=None, font_size=None):
        if word_pos is None or font_size is None or len(word_pos) == 0:
            self._chk(self.lib.rt_set_fontsize(self.h, None, None, 0))
            return
        wp = [int(v) for v in word_pos.tolist()]
        fs = [float(v) for v in font_size.tolist()]
        self._chk(self.lib.rt_set_fontsize(self.h, (C.c_int64 * len(wp))(*wp), (C.c_float * len(fs))(*fs), len(wp)))

    def set_schedule(self, kind, timesteps, table, num_inference_steps):
        ts = [float(v) for v in timesteps]
        tb = [float(v) for v in table]
        self._chk(self.lib.rt_set_schedule(self.h, kind, (C.c_float * len(ts))(*ts), len(ts), (C.c_float * len(tb))(*tb),
                                           len(tb), num_inference_steps))

    def set_noise_seed(self, seed):
        """Key of the per-step noise field of the stochastic samplers (schedule kinds 4 / 5 / 6); None = 0.  Engine state: it survives
        set_schedule / set_latents, and the deterministic kinds ignore it."""
        self._chk(self.lib.rt_set_noise_seed(self.h, C.c_uint64(int(seed or 0) & 0xFFFFFFFFFFFFFFFF)))

    def set_prediction(self, prediction_type=PRED_EPSILON, guidance_rescale=0.0):
        """What the UNet predicts (0 / 'epsilon', 1 / 'v_prediction') and the CFG rescale phi in [0, 1].  Engine state, default (0, 0),
        under which a step launches what it always launched; otherwise the two launches of csrc/guided.hip run before the step epilogue
        (include/rtdiff.h: rt_set_prediction).  Survives set_schedule / set_latents; a bad value raises and changes nothing."""
        if isinstance(prediction_type, str):
            if prediction_type not in PREDICTION_TYPES:
                raise ValueError(f"prediction_type must be one of {sorted(PREDICTION_TYPES)}, got {prediction_type!r}")
            prediction_type = PREDICTION_TYPES[prediction_type]
        self._chk(self.lib.rt_set_prediction(self.h, int(prediction_type), C.c_float(float(guidance_rescale))))

    def set_freeu(self, s1, s2, b1, b2):
        """FreeU in the first two up blocks (include/rtdiff.h: rt_set_freeu; diffusers' argument order): the four lowest frequency bins of
        the skip features times s1 / s2, half of the backbone channels times b1 / b2.  All finite and > 0; (1, 1, 1, 1) = off, under
        which a forward launches what it always launched.  Engine state: it holds until set again; a bad value raises and changes nothing."""
        self._chk(self.lib.rt_set_freeu(self.h, C.c_float(float(s1)), C.c_float(float(s2)), C.c_float(float(b1)), C.c_float(float(b2))))

    def disable_freeu(self):
        self.set_freeu(1.0, 1.0, 1.0, 1.0)

    def set_latents(self, latents):
        l = latents.contiguous().float()
        assert l.shape[0] == 1 and l.shape[1] == 4
        self._chk(self.lib.rt_set_latents(self.h, _ptr(l), l.shape[2], l.shape[3]))
        self.synchronize()

    # ---- image start: the source (encoded image + noise + optional keep mask), its noised start and the per-step pin
    def set_source(self, x0, noise=None, keep=None):
        """x0, noise [1,4,h,w]; keep [h,w] or [1,1,h,w] in [0,1] or None (nothing pinned).  x0 None clears the source."""
        if x0 is None:
            self._chk(self.lib.rt_set_source(self.h, None, None, None, 0, 0))
            return
        x0, noise = x0.contiguous().float(), noise.contiguous().float()
        h, w = x0.shape[-2], x0.shape[-1]
        assert tuple(x0.shape) == (1, 4, h, w) and noise.shape == x0.shape, (tuple(x0.shape), tuple(noise.shape))
        if keep is not None:
            keep = keep.contiguous().float()
            assert keep.numel() == h * w and tuple(keep.shape[-2:]) == (h, w), tuple(keep.shape)
        self._chk(self.lib.rt_set_source(self.h, _ptr(x0), _ptr(noise), _ptr(keep), h, w))
        self.synchronize()

    def noise_latents(self, a, b):
        self._chk(self.lib.rt_noise_latents(self.h, C.c_float(float(a)), C.c_float(float(b))))

    def source_blend(self, a, b):
        self._chk(self.lib.rt_source_blend(self.h, C.c_float(float(a)), C.c_float(float(b))))

    # ---- token-map attention store
    def attn_modules(self):
        n = self.lib.rt_attn_module_count(self.h)
        name = C.create_string_buffer(256)
        mt, hd = C.c_int(), C.c_int()
        out = []
        for i in range(n):
            self._chk(self.lib.rt_attn_module_info(self.h, i, name, 256, C.byref(mt), C.byref(hd)))
            out.append((name.value.decode(), mt.value, hd.value))
        return out

    def attn_store_enable(self, name, mode=1):
        self._chk(self.lib.rt_attn_store_enable(self.h, name.encode(), int(mode)))

    def attn_store_reset(self):
        self._chk(self.lib.rt_attn_store_reset(self.h))

    def attn_store_read(self, name):
        """-> (n_calls, map [1, rows, cols] on the GPU or None if nothing was recorded yet)"""
        import torch
        n, r, c = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.lib.rt_attn_store_read(self.h, name.encode(), None, C.byref(n), C.byref(r), C.byref(c)))
        if r.value == 0:
            return n.value, None
        out = torch.empty(1, r.value, c.value, device=f"cuda:{self.device}")
        self._chk(self.lib.rt_attn_store_read(self.h, name.encode(), _ptr(out), C.byref(n), C.byref(r), C.byref(c)))
        return n.value, out

    def state_ptrs(self):
        """Device pointers of the sampler state: (latents [4,h,w], CFG-combined noise_pred of the last rich step)."""
        a, b = C.c_void_p(), C.c_void_p()
        self._chk(self.lib.rt_get_state_ptrs(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- profiling (HIP events around every MFMA kernel launch on the engine stream)
    PROF_CLASSES = {0: "gemm_kernel<A_DENSE>", 1: "gemm_kernel<A_CONV3*>", 2: "attn_kernel<self>", 3: "attn_kernel<cross>",
                    5: "gemm16_kernel<EPI_XATTN> (to_q + cross-attention)", 6: "xblock_kernel (to_q + cross-attention + to_out)"}
    PROF_STORE = 4          # attn_store_kernel (plain pass, token-map capture) and, with set_freeu on, the FreeU launches: priced in algorithmic HBM bytes

    def profile_read_store(self):
        n, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
        self._chk(self.lib.rt_profile_read2(self.h, self.PROF_STORE, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)))
        return dict(launches=n.value, total_ms=ms.value, total_flops=fl.value, total_bytes=by.value)

    PROF_IP = 7             # ipattn_kernel (the image-prompt term of attn2, set_image_prompts): FLOPs and algorithmic HBM bytes

    def profile_read_ip(self):
        n, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
        self._chk(self.lib.rt_profile_read2(self.h, self.PROF_IP, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)))
        return dict(launches=n.value, total_ms=ms.value, total_flops=fl.value, total_bytes=by.value)

    def profile_enable(self, on=True):
        self._chk(self.lib.rt_profile_enable(self.h, int(on)))

    def profile_read(self):
        out = {}
        for cls, name in self.PROF_CLASSES.items():
            n, ms, fl = C.c_int(), C.c_double(), C.c_double()
            self._chk(self.lib.rt_profile_read(self.h, cls, C.byref(n), C.byref(ms), C.byref(fl)))
            out[name] = dict(launches=n.value, total_ms=ms.value, total_flops=fl.value)
        return out

    def read_latents(self, h, w, with_ref=False):
        import torch
        out = torch.empty(1, 4, h, w, device=f"cuda:{self.device}")
        ref = torch.empty_like(out) if with_ref else None
        self._chk(self.lib.rt_get_latents(self.h, _ptr(out), _ptr(ref)))
        self.synchronize()
        return (out, ref) if with_ref else out

    # ---- hot path
    def region_step(self, i, guidance_scale, inject_selfattn=0.0, inject_background=0.0, xl=True, elide=False, defer_blend=False):
        self._chk(self.lib.rt_region_step(self.h, i, C.c_float(guidance_scale), C.c_double(inject_selfattn),
                                          C.c_double(inject_background), int(xl), int(bool(elide)) | (2 if defer_blend else 0)))

    # ---- intra-image split of a step over the ranks of a process group (launcher.split_region_step drives these)
    def region_step_part(self, i, guidance_scale, inject_selfattn, inject_background, xl, part, nparts, elide=False, defer_blend=False):
        """The UNet forwards of this rank's contiguous stream range of step i -> (first_stream, n_streams, (streams of the step, its
        text_ref stream or -1, injection on))."""
        first, count, info = C.c_int(), C.c_int(), (C.c_int * 3)()
        self._chk(self.lib.rt_region_step_part(self.h, i, C.c_float(guidance_scale), C.c_double(inject_selfattn), C.c_double(inject_background),
                                               int(xl), int(bool(elide)) | (2 if defer_blend else 0), part, nparts, C.byref(first), C.byref(count), info))
        return first.value, count.value, (info[0], info[1], bool(info[2]))

    def region_step_finish(self, i, guidance_scale, inject_selfattn, inject_background, xl, elide=False, defer_blend=False):
        self._chk(self.lib.rt_region_step_finish(self.h, i, C.c_float(guidance_scale), C.c_double(inject_selfattn), C.c_double(inject_background),
                                                 int(xl), int(bool(elide)) | (2 if defer_blend else 0)))

    def eps_info(self):
        """(device pointer, bytes per stream, max streams) of the noise-prediction buffer [max_streams][h*w][4] fp32."""
        p, b, m = C.c_void_p(), C.c_uint64(), C.c_int()
        self._chk(self.lib.rt_eps_info(self.h, C.byref(p), C.byref(b), C.byref(m)))
        return p.value, b.value, m.value

    def background_blend(self):
        self._chk(self.lib.rt_background_blend(self.h))

    def plain_step(self, i, guidance_scale):
        self._chk(self.lib.rt_plain_step(self.h, i, C.c_float(guidance_scale)))

    def plain_step_part(self, i, part, nparts):
        """The forwards of this rank's range of the plain step's streams [uncond, text] (launcher.split_plain_step); returns (first, count)."""
        first, count = C.c_int(0), C.c_int(0)
        self._chk(self.lib.rt_plain_step_part(self.h, i, part, nparts, C.byref(first), C.byref(count)))
        return first.value, count.value

    def plain_streams(self):
        """The streams of a plain step as the state stands: 2, or 3 with a perturbed twin of the text stream (set_pag_scales)."""
        n = C.c_int(0)
        self._chk(self.lib.rt_plain_streams(self.h, C.byref(n)))
        return n.value

    def plain_step_finish(self, i, guidance_scale):
        self._chk(self.lib.rt_plain_step_finish(self.h, i, C.c_float(guidance_scale)))

    def trace_modules(self):
        """The modules whose trunk tensor unet_forward(..., trace=name) can read, in execution order: [(name, channels, downshift)]
        (include/rtdiff.h: rt_trace_module_info; the module's grid is the latent grid >> downshift).  Needs no device."""
        n = self.lib.rt_trace_module_count(self.h)
        name = C.create_string_buffer(256)
        ch, sh = C.c_int(), C.c_int()
        out = []
        for i in range(n):
            self._chk(self.lib.rt_trace_module_info(self.h, i, name, 256, C.byref(ch), C.byref(sh)))
            out.append((name.value.decode(), ch.value, sh.value))
        return out

    def unet_forward(self, x, timestep, prompt_idx, in_scale=None, fontsize=None, qk_src=None, res_src=None, trace=None, perturb=None):
        """perturb = per stream 1 / 0: the stream is perturbed at the applied modules of set_pag_layers (rt_unet_forward_perturbed; the
        perturbed streams trail the list).  trace = a module name of trace_modules(): returns (out, the trunk tensor that module leaves as fp32 [B, C, h', w']) - the same
        forward, `out` bit for bit (rt_unet_forward_trace: test infrastructure)."""
        import torch
        x = x.contiguous().float()
        B, _, h, w = x.shape
        out = torch.empty_like(x)

        def iarr(v):
            return (C.c_int * B)(*[int(k) for k in v]) if v is not None else None
        sc = (C.c_float * B)(*[float(k) for k in in_scale]) if in_scale is not None else None
        if trace is not None:
            shapes = {n: (c, s) for n, c, s in self.trace_modules()}
            if trace not in shapes:
                raise RtError(-1, f"unet_forward: not a traceable module: {trace}")
            ch, sh = shapes[trace]
            tr = torch.empty(B, ch, h >> sh, w >> sh, device=x.device)
            if trace.startswith("controlnet."):      # the control copy's own modules leave the CONTROLLED streams only, the hint embedding one entry: the rest stays NaN
                tr.fill_(float("nan"))
            if perturb is not None:
                self._chk(self.lib.rt_unet_forward_perturbed(self.h, _ptr(x), B, h, w, C.c_float(float(timestep)), sc, iarr(prompt_idx), iarr(fontsize),
                                                             iarr(qk_src), iarr(res_src), _ptr(out), trace.encode(), _ptr(tr), C.c_longlong(tr.numel()),
                                                             iarr(perturb)))
            else:
                self._chk(self.lib.rt_unet_forward_trace(self.h, _ptr(x), B, h, w, C.c_float(float(timestep)), sc, iarr(prompt_idx), iarr(fontsize),
                                                         iarr(qk_src), iarr(res_src), _ptr(out), trace.encode(), _ptr(tr), C.c_longlong(tr.numel())))
            self.synchronize()
            return out, tr
        if perturb is not None:
            self._chk(self.lib.rt_unet_forward_perturbed(self.h, _ptr(x), B, h, w, C.c_float(float(timestep)), sc, iarr(prompt_idx), iarr(fontsize),
                                                         iarr(qk_src), iarr(res_src), _ptr(out), None, None, C.c_longlong(0), iarr(perturb)))
            self.synchronize()
            return out
        self._chk(self.lib.rt_unet_forward(self.h, _ptr(x), B, h, w, C.c_float(float(timestep)), sc, iarr(prompt_idx),
                                           iarr(fontsize), iarr(qk_src), iarr(res_src), _ptr(out)))
        self.synchronize()
        return out


def step_noise(seed, step, h, w, words=False, device=0):
    """The N(0, 1) field a stochastic step with (noise seed, step index) adds on an h x w latent grid, from the device function the step
    epilogue calls: [1, 4, h, w] fp32 on the GPU; words=True also returns the raw Philox words [h*w, 4] (uint32 bit patterns in int64)."""
    import torch
    lib = load_library()
    dev = f"cuda:{device}"
    with torch.cuda.device(dev):
        out = torch.empty(1, 4, h, w, device=dev)
        wd = torch.empty(h * w, 4, dtype=torch.int32, device=dev) if words else None
        rc = lib.rt_op_step_noise(C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(step), int(h), int(w), _ptr(out), _ptr(wd),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RtError(rc, lib.rt_op_last_error().decode())
        torch.cuda.synchronize()
    return (out, wd.to(torch.int64) & 0xFFFFFFFF) if words else out


def ip_attention(Q, Kip, VTip, O, slots, counts, scales, H, N, DP):
    """The image-prompt term of decoupled cross-attention alone (rt_op_ip_attention), IN PLACE on O: bf16 2-D tensors (views with a row
    stride are fine: the stride is the leading dimension) Q / O [B N, >= H DP], Kip [16 slots, >= H DP], VTip [H DP, >= 16 slots]; per
    batch entry a slot (-1: skipped), its valid keys (1 .. 16) and the scale (0: skipped).  Returns O."""
    import torch
    lib = load_library()
    B = len(slots)
    for t in (Q, Kip, VTip, O):
        assert t.dtype == torch.bfloat16 and t.dim() == 2 and t.stride(1) == 1 and t.device == O.device, "ip_attention: bf16 [rows, ld] tensors on one device"
    assert len(counts) == B and len(scales) == B and Q.shape[0] >= B * N and O.shape[0] >= B * N, "ip_attention: batch"
    assert VTip.shape[0] >= H * DP and min(Q.shape[1], O.shape[1], Kip.shape[1]) >= H * DP, "ip_attention: widths"
    assert all(s < 0 or (16 * (s + 1) <= Kip.shape[0] and 16 * (s + 1) <= VTip.shape[1]) for s in slots), "ip_attention: slot outside the caches"
    with torch.cuda.device(O.device):
        rc = lib.rt_op_ip_attention(_ptr(Q), int(Q.stride(0)), _ptr(Kip), int(Kip.stride(0)), _ptr(VTip), int(VTip.stride(0)), _ptr(O), int(O.stride(0)),
                                    (C.c_int * B)(*[int(v) for v in slots]), (C.c_int * B)(*[int(v) for v in counts]),
                                    (C.c_float * B)(*[float(v) for v in scales]), B, int(H), int(N), int(DP),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RtError(rc, lib.rt_op_last_error().decode())
        torch.cuda.synchronize()
    return O


def identity_attention(VT, O, entries, H, N, DP):
    """The identity attention of perturbed-attention guidance alone (rt_op_identity_attention), on the caller's bf16 2-D tensors (views with
    a row stride are fine: the stride is the leading dimension): O[b N + n, c] = VT[c, b N + n] for c < H DP and the batch entries named;
    VT [H DP, >= B N], O [B N, >= H DP].  Returns O."""
    import torch
    lib = load_library()
    for t in (VT, O):
        assert t.dtype == torch.bfloat16 and t.dim() == 2 and t.stride(1) == 1 and t.device == O.device, "identity_attention: bf16 [rows, ld] tensors on one device"
    assert VT.shape[0] >= H * DP and O.shape[1] >= H * DP and N >= 1 and O.shape[0] % N == 0 and VT.shape[1] >= O.shape[0], "identity_attention: shapes"
    n = len(entries)
    with torch.cuda.device(O.device):
        rc = lib.rt_op_identity_attention(_ptr(VT), int(VT.stride(0)), _ptr(O), int(O.stride(0)), (C.c_int * max(1, n))(*[int(v) for v in entries]), n,
                                          int(O.shape[0] // N), int(H), int(N), int(DP), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RtError(rc, lib.rt_op_last_error().decode())
        torch.cuda.synchronize()
    return O


def pag_fold(eps, h, w, streams, twins, ratios):
    """The fold of a step alone (rt_op_pag_fold), IN PLACE on eps [F, h w, 4] fp32 (contiguous, the engine's eps layout):
    eps[streams[i]] <- fmaf(ratios[i], eps[streams[i]] - eps[twins[i]], eps[streams[i]]).  Returns eps."""
    import torch
    lib = load_library()
    assert eps.dtype == torch.float32 and eps.is_contiguous() and eps.dim() == 3 and eps.shape[1] == h * w and eps.shape[2] == 4, "pag_fold: fp32 [F, h w, 4]"
    n = len(streams)
    assert len(twins) == n and len(ratios) == n
    with torch.cuda.device(eps.device):
        rc = lib.rt_op_pag_fold(_ptr(eps), int(eps.shape[0]), int(h), int(w), (C.c_int * max(1, n))(*[int(v) for v in streams]),
                                (C.c_int * max(1, n))(*[int(v) for v in twins]), (C.c_float * max(1, n))(*[float(v) for v in ratios]), n,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RtError(rc, lib.rt_op_last_error().decode())
        torch.cuda.synchronize()
    return eps


LORA_FORMS = {"bf16": 0, "bf16_t": 1, "f16": 2}


def lora_add(X, down, up, alpha_over_rank, col_adapter, Y, form, rows_at, scales, rows):
    """The unmerged low-rank term of one projection alone (rt_op_lora_add), IN PLACE on Y: per batch entry b with its `rows` rows at
    rows_at[b] and the adapter scales scales[b] (up to 4), Y += bf16(f_b (X down^T)) up^T, f_b[j] = scales[b][col_adapter[j]] *
    alpha_over_rank[j].  X [*, >= K], down [R, >= K], up [N, >= R] bf16 2-D tensors (views with a row stride are fine: the stride is the
    leading dimension), alpha_over_rank [R] fp32, col_adapter [R] int32; form "bf16": Y bf16 [*, >= N]; "bf16_t": Y bf16 [N, >= columns]
    holding the transpose, entry b at columns rows_at[b] ...; "f16": Y fp16 [*, >= N].  An entry whose scales are all 0 is skipped.
    Returns the number of entries launched."""
    import torch
    lib = load_library()
    f = LORA_FORMS[form]
    B = len(rows_at)
    R, K = down.shape
    N = up.shape[0]
    for t in (X, down, up, Y):
        assert t.dim() == 2 and t.stride(1) == 1 and t.device == Y.device, "lora_add: [rows, ld] tensors on one device"
    assert X.dtype == down.dtype == up.dtype == torch.bfloat16 and Y.dtype == (torch.float16 if f == 2 else torch.bfloat16), "lora_add: dtypes"
    assert alpha_over_rank.dtype == torch.float32 and col_adapter.dtype == torch.int32 and alpha_over_rank.numel() == R == col_adapter.numel() == up.shape[1]
    assert alpha_over_rank.is_contiguous() and col_adapter.is_contiguous() and X.shape[1] >= K and len(scales) == B
    top = max(int(r) for r in rows_at) + rows
    assert X.shape[0] >= top and (Y.shape[1] >= top and Y.shape[0] >= N if f == 1 else Y.shape[0] >= top and Y.shape[1] >= N), "lora_add: a stream outside the tensors"
    sc = [float(s[l]) if l < len(s) else 0.0 for s in scales for l in range(4)]
    n = C.c_int(0)
    with torch.cuda.device(Y.device):
        rc = lib.rt_op_lora_add(_ptr(X), int(X.stride(0)), _ptr(down), int(down.stride(0)), _ptr(up), int(up.stride(0)), _ptr(alpha_over_rank),
                                _ptr(col_adapter), _ptr(Y), int(Y.stride(0)), f, (C.c_int * B)(*[int(v) for v in rows_at]), (C.c_float * (4 * B))(*sc),
                                B, int(rows), int(K), int(N), int(R), C.byref(n), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RtError(rc, lib.rt_op_last_error().decode())
        torch.cuda.synchronize()
    return n.value


def lora_geglu(X, down, up, alpha_over_rank, col_adapter, Z, out, rows_at, scales, rows):
    """ff.net.0.proj of adapted streams from the base projection's fp32 pre-activations (rt_op_lora_geglu): per batch entry b with its `rows`
    rows at rows_at[b] and the adapter scales scales[b], out = bf16((Zv + Dv) gelu(Zg + Dg)) with D = bf16(f_b (X down^T)) up^T.  X [*, >= K],
    down [R, >= K], up [N, >= R] (rows in the packed GEGLU order) bf16, Z [*, >= N] fp32 (packed columns, per 64 [32 value | 32 gate]),
    out [*, >= N / 2] bf16; 2-D tensors whose row stride is the leading dimension.  An entry whose scales are all 0 is skipped and its rows
    of out are not written.  Returns the number of entries launched."""
    import torch
    lib = load_library()
    B = len(rows_at)
    R, K = down.shape
    N = up.shape[0]
    for t in (X, down, up, Z, out):
        assert t.dim() == 2 and t.stride(1) == 1 and t.device == out.device, "lora_geglu: [rows, ld] tensors on one device"
    assert X.dtype == down.dtype == up.dtype == out.dtype == torch.bfloat16 and Z.dtype == torch.float32, "lora_geglu: dtypes"
    assert alpha_over_rank.dtype == torch.float32 and col_adapter.dtype == torch.int32 and alpha_over_rank.numel() == R == col_adapter.numel() == up.shape[1]
    assert alpha_over_rank.is_contiguous() and col_adapter.is_contiguous() and X.shape[1] >= K and len(scales) == B
    top = max(int(r) for r in rows_at) + rows
    assert min(X.shape[0], Z.shape[0], out.shape[0]) >= top and Z.shape[1] >= N and out.shape[1] >= N // 2, "lora_geglu: a stream outside the tensors"
    sc = [float(s[l]) if l < len(s) else 0.0 for s in scales for l in range(4)]
    n = C.c_int(0)
    with torch.cuda.device(out.device):
        rc = lib.rt_op_lora_geglu(_ptr(X), int(X.stride(0)), _ptr(down), int(down.stride(0)), _ptr(up), int(up.stride(0)), _ptr(alpha_over_rank),
                                  _ptr(col_adapter), _ptr(Z), int(Z.stride(0)), _ptr(out), int(out.stride(0)), (C.c_int * B)(*[int(v) for v in rows_at]),
                                  (C.c_float * (4 * B))(*sc), B, int(rows), int(K), int(N), int(R), C.byref(n),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RtError(rc, lib.rt_op_last_error().decode())
        torch.cuda.synchronize()
    return n.value


def freeu(hidden, skip, H, W, b=1.0, s=1.0):
    """The FreeU operator alone (rt_op_freeu), IN PLACE on the caller's fp16 token-major tensors: hidden [B, H W, C1] - channels
    < C1 // 2 times b - and skip [B, H W, C2] - the four lowest frequency bins of every (stream, channel) map times s.  Either may be
    None; b == 1 / s == 1 launch nothing for their half.  Returns (hidden, skip)."""
    import torch
    lib = load_library()
    ref = hidden if hidden is not None else skip
    for t in (hidden, skip):
        assert t is None or (t.dtype == torch.float16 and t.dim() == 3 and t.is_contiguous() and t.shape[1] == H * W and t.device == ref.device), \
            "freeu: contiguous fp16 [B, H W, C] tensors on one device"
    assert hidden is None or skip is None or hidden.shape[0] == skip.shape[0], "freeu: hidden and skip differ in streams"
    with torch.cuda.device(ref.device):
        rc = lib.rt_op_freeu(_ptr(hidden), int(hidden.shape[2]) if hidden is not None else 0, _ptr(skip),
                             int(skip.shape[2]) if skip is not None else 0, int(ref.shape[0]), int(H), int(W), C.c_float(float(b)),
                             C.c_float(float(s)), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RtError(rc, lib.rt_op_last_error().decode())
        torch.cuda.synchronize()
    return hidden, skip


def control_add(skip, r, streams, scales, C_=None):
    """The ControlNet residual add alone (rt_op_control_add), IN PLACE on skip: fp16 [B, HW, >= C] (a view with row / stream strides is
    fine: they are the leading dimension and the stream stride), r fp32 [n, HW, >= C]; entry i adds scales[i] * r[i] into stream
    streams[i].  C_ = the channel count when the tensors are wider views (default: skip's last dimension).  Returns skip."""
    import torch
    lib = load_library()
    n = len(streams)
    assert skip.dtype == torch.float16 and r.dtype == torch.float32 and skip.dim() == 3 and r.dim() == 3, "control_add: fp16 [B, HW, C] and fp32 [n, HW, C]"
    assert skip.stride(2) == 1 and r.stride(2) == 1 and skip.device == r.device and r.shape[0] >= n and len(scales) == n and r.shape[1] == skip.shape[1]
    Cc = int(C_ or skip.shape[2])
    assert Cc <= skip.shape[2] and Cc <= r.shape[2]
    with torch.cuda.device(skip.device):
        rc = lib.rt_op_control_add(_ptr(skip), C.c_longlong(skip.stride(0)), int(skip.stride(1)), _ptr(r), C.c_longlong(r.stride(0)), int(r.stride(1)),
                                   (C.c_int * max(1, n))(*[int(v) for v in streams]), (C.c_float * max(1, n))(*[float(v) for v in scales]), n,
                                   int(skip.shape[0]), int(skip.shape[1]), Cc, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RtError(rc, lib.rt_op_last_error().decode())
        torch.cuda.synchronize()
    return skip


def guided_prediction(eps, lat, g, s_uncond=0, s_base=1, masks=None, lat_ref=None, s_uref=-1, s_tref=-1, s_region=(), plain=True,
                      step_ref=False, guidance_rescale=0.0, prediction_type=PRED_EPSILON, cv=1.0, cx=0.0):
    """The guided-prediction pre-pass alone (rt_op_guided_prediction), on the caller's tensors: eps [F, h*w, 4] fp32 (the layout of the
    engine's eps buffer), lat / lat_ref [1, 4, h, w], masks [R, 4, h, w] (rich mode) -> (gpred [2, h*w, 4], factors [2]) on the GPU.
    Slot 1 of gpred is only written when the reference pair is stepped (s_uref >= 0 and step_ref)."""
    import torch
    lib = load_library()
    dev = eps.device
    h, w = lat.shape[-2], lat.shape[-1]
    eps, lat = eps.contiguous().float(), lat.contiguous().float()
    assert eps.dim() == 3 and tuple(eps.shape[1:]) == (h * w, 4), tuple(eps.shape)
    assert max(s_uncond, s_base, s_uref, s_tref, *s_region) < eps.shape[0], "a stream index lies outside eps"
    lat_ref = lat_ref.contiguous().float() if lat_ref is not None else None
    R = 0
    if not plain:
        masks = masks.contiguous().float()
        R = masks.shape[0]
        assert tuple(masks.shape) == (R, 4, h, w) and len(s_region) == R - 1, (tuple(masks.shape), len(s_region))
    with torch.cuda.device(dev):
        gpred = torch.full((2, h * w, 4), float("nan"), device=dev)
        factors = torch.empty(2, device=dev)
        partials = torch.empty(-(-h * w // 256) * 8, dtype=torch.float64, device=dev)
        reg = (C.c_int * max(1, len(s_region)))(*[int(v) for v in s_region])
        rc = lib.rt_op_guided_prediction(_ptr(eps), _ptr(masks if not plain else None), _ptr(lat), _ptr(lat_ref), int(h), int(w), int(R),
                                         int(s_uncond), int(s_base), int(s_uref), int(s_tref), reg, C.c_float(float(g)), int(bool(plain)),
                                         int(bool(step_ref)), C.c_float(float(guidance_rescale)), int(prediction_type), C.c_float(float(cv)),
                                         C.c_float(float(cx)), _ptr(gpred), _ptr(partials), _ptr(factors),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
        if rc != 0:
            raise RtError(rc, lib.rt_op_last_error().decode())
        torch.cuda.synchronize()
    return gpred, factors


# ------------------------------------------------------------------------------------------------ VAE decoder
SD_VAE_CONFIG = dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2, norm_num_groups=32, scaling_factor=0.18215)
SDXL_VAE_CONFIG = dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2, norm_num_groups=32, scaling_factor=0.13025)


class RtVaeConfig(C.Structure):
    _fields_ = [("n_blocks", C.c_int), ("block_out_channels", C.c_int * RT_MAX_LEVELS), ("layers_per_block", C.c_int),
                ("norm_groups", C.c_int), ("scaling_factor", C.c_float), ("latent_h", C.c_int), ("latent_w", C.c_int),
                ("precise", C.c_int)]


_VAE_ALIASES = ((".to_q.", ".query."), (".to_k.", ".key."), (".to_v.", ".value."), (".to_out.0.", ".proj_attn."))


class _VaeHandle:
    """ctypes plumbing shared by the two roles of an rt_vae handle (decoder / encoder): config, weight table, binding, lifetime."""
    _create = "rt_vae_create"

    def __init__(self, cfg, latent_h, latent_w, device=0, state_dict=None, precise=False):
        self.lib = load_library()
        c = RtVaeConfig()
        boc = tuple(cfg["block_out_channels"])
        c.n_blocks = len(boc)
        for i, v in enumerate(boc):
            c.block_out_channels[i] = v
        c.layers_per_block = cfg["layers_per_block"]
        c.norm_groups = cfg["norm_num_groups"]
        c.scaling_factor = cfg["scaling_factor"]
        c.latent_h, c.latent_w = latent_h, latent_w
        c.precise = int(bool(precise))
        self.precise = bool(precise)
        self.cfg, self.cfg_dict, self.device = c, dict(cfg), device
        self.scaling_factor = cfg["scaling_factor"]
        self.h = C.c_void_p()
        rc = getattr(self.lib, self._create)(C.byref(c), device, C.byref(self.h))
        if rc != 0:
            raise RtError(rc, self.lib.rt_vae_last_error(None).decode())
        if state_dict is not None:
            self.load_state_dict(state_dict)

    def _chk(self, rc):
        if rc != 0:
            raise RtError(rc, self.lib.rt_vae_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.rt_vae_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def weight_table(self):
        n = self.lib.rt_vae_weight_count(self.h)
        name = C.create_string_buffer(256)
        shape, nd = (C.c_int64 * 4)(), C.c_int()
        out = []
        for i in range(n):
            self._chk(self.lib.rt_vae_weight_info(self.h, i, name, 256, shape, C.byref(nd)))
            out.append((name.value.decode(), tuple(shape[k] for k in range(nd.value))))
        return out

    def load_state_dict(self, sd):
        """Binds the handle's weights from `sd` (AutoencoderKL state-dict names; keys of the other role are ignored)."""
        import torch
        dev = f"cuda:{self.device}"
        for name, _ in self.weight_table():
            key = name
            if key not in sd:                       # pre-0.18 AttentionBlock names of older checkpoints
                for new, old in _VAE_ALIASES:
                    key = key.replace(new, old)
            t = sd[key].to(dev).contiguous()
            dt = {torch.float32: DTYPE_F32, torch.float16: DTYPE_F16, torch.bfloat16: DTYPE_BF16}[t.dtype]
            shape = (C.c_int64 * max(1, t.dim()))(*t.shape)
            self._chk(self.lib.rt_vae_bind_weight(self.h, name.encode(), _ptr(t), dt, shape, t.dim()))
        self._chk(self.lib.rt_vae_synchronize(self.h))

    def arena(self):
        p, b = C.c_void_p(), C.c_uint64()
        self._chk(self.lib.rt_vae_arena_info(self.h, C.byref(p), C.byref(b)))
        return p.value, b.value

    def arena_mark_bound(self):
        self._chk(self.lib.rt_vae_arena_mark_bound(self.h))

    def synchronize(self):
        self._chk(self.lib.rt_vae_synchronize(self.h))


class VaeDecoder(_VaeHandle):
    """AutoencoderKL decoder on the engine: `.decode(z)` (same call surface as diffusers' `vae.decode(z).sample`) and
    the colour-guidance update of the rich-text loop (rd.py:151-168 / xl.py:849-867).

    `precise=True` runs every contraction as three bf16 MFMA passes over (hi, lo) operand pairs - fp32-class products - which is
    what the SDXL pipeline of the reference asks of its VAE (xl.py:856 `.to(dtype=torch.float32)`); the SD pipeline decodes in the
    checkpoint's dtype (rd.py:160) and keeps the single-pass default."""

    def decode(self, z, divide_by_scaling=False):
        """z [1,4,h,w] -> image [1,3,8h,8w] in [-1,1]"""
        import torch
        z = z.contiguous().float()
        _, _, h, w = z.shape
        out = torch.empty(1, 3, 8 * h, 8 * w, device=z.device)
        self._chk(self.lib.rt_vae_decode(self.h, _ptr(z), h, w, int(divide_by_scaling), _ptr(out)))
        return out

    def color_guidance(self, latents_ptr_or_tensor, noise_pred, alpha_t, h, w, color_obj_atten, target_rgb, weight, color_obj_atten_all,
                       want_grad=False):
        """In-place update of `latents` (tensor [1,4,h,w] or raw device pointer) exactly as rd.py:151-168."""
        import torch
        # the masks / targets are the same objects on every step of a loop (sample.py:87-88 builds them once): stage them on the
        # device once instead of per step (image-resolution masks from pageable host memory are a synchronous multi-MB copy)
        # the reference pairs masks and targets with zip() (rd.py:158): sample.py hands over n_color + 1 masks (get_token_maps
        # appends the background mask) but n_color targets, so the surplus mask is silently dropped.  Same here.
        n = min(len(color_obj_atten), len(target_rgb))
        if n == 0:
            raise RtError(-1, "color_guidance: no (mask, target RGB) pair")
        key = (id(color_obj_atten), id(target_rgb), id(color_obj_atten_all), n)
        if getattr(self, "_cg_key", None) != key:
            masks = torch.cat([m[:, 0].reshape(1, -1) for m in color_obj_atten[:n]]).contiguous().float().to(f"cuda:{self.device}")
            tgt = [float(v) for t in target_rgb[:n] for v in t.flatten().tolist()]
            if len(tgt) != 3 * n or masks.shape != (n, 64 * h * w):
                raise RtError(-1, f"color_guidance: need {n} RGB triples and [{n}, {64 * h * w}] masks, got {len(tgt)} values / {tuple(masks.shape)}")
            mall = color_obj_atten_all.contiguous().float().to(f"cuda:{self.device}")
            self._cg_key, self._cg_val = key, (masks, (C.c_float * len(tgt))(*tgt), mall, (color_obj_atten, target_rgb, color_obj_atten_all))
        masks, tgt_arr, mall, _ = self._cg_val
        grad = torch.empty(1, 4, h, w, device=f"cuda:{self.device}") if want_grad else None
        loss = C.c_float()
        lp = latents_ptr_or_tensor if isinstance(latents_ptr_or_tensor, int) else latents_ptr_or_tensor.data_ptr()
        npp = noise_pred if isinstance(noise_pred, int) else noise_pred.data_ptr()
        self._chk(self.lib.rt_vae_color_guidance(self.h, C.c_void_p(lp), C.c_void_p(npp), C.c_float(float(alpha_t)), h, w, _ptr(masks),
                                                 tgt_arr, n, C.c_float(float(weight)), _ptr(mall),
                                                 _ptr(grad), C.byref(loss)))
        return loss.value, grad


class VaeEncoder(_VaeHandle):
    """AutoencoderKL encoder + quant_conv on the engine (diffusers 0.18.2 call surface: `encode(x).latent_dist.sample()`), for
    RegionDiffusion.encode_imgs (rd.py:238-246).  The plan takes images up to 8 latent_h x 8 latent_w (H, W multiples of 8);
    `state_dict` may be a full AutoencoderKL state dict: only its `encoder.*` / `quant_conv.*` keys are read.  `precise` as VaeDecoder."""
    _create = "rt_vae_encoder_create"

    def __init__(self, cfg, latent_h, latent_w, device=0, state_dict=None, precise=False):
        if cfg.get("latent_channels", 4) != 4:
            raise ValueError("VaeEncoder: latent_channels must be 4")
        self.factor = 2 ** (len(cfg["block_out_channels"]) - 1)
        super().__init__(cfg, latent_h, latent_w, device, state_dict, precise)

    def encode(self, x, in_scale=1.0, in_shift=0.0):
        """x [B,3,H,W] -> object with `.latent_dist` (DiagonalGaussianDistribution of the moments of in_scale * x + in_shift).
        One image per rt_vae_encode call."""
        import torch
        x = x.to(f"cuda:{self.device}").float().contiguous()
        B, ch, H, W = x.shape
        if ch != 3:
            raise ValueError(f"VaeEncoder.encode: expected [B, 3, H, W], got {tuple(x.shape)}")
        mom = torch.empty(B, 8, H // self.factor, W // self.factor, device=x.device)
        for b in range(B):
            self._chk(self.lib.rt_vae_encode(self.h, _ptr(x[b]), H, W, C.c_float(float(in_scale)), C.c_float(float(in_shift)), _ptr(mom[b])))
        return EncoderOutput(DiagonalGaussianDistribution(self, mom))


class DiagonalGaussianDistribution:
    """diffusers' posterior over the moments [B, 8, h, w] (mean | logvar clamped to [-30, 20] by the encode kernel)."""

    def __init__(self, encoder, moments):
        self.encoder, self.moments = encoder, moments
        self.mean, self.logvar = moments[:, :4], moments[:, 4:]

    def mode(self):
        return self.mean

    def sample(self, generator=None, scale=1.0):
        """scale * (mean + exp(0.5 logvar) * eps), eps from ONE torch.randn call for the batch (diffusers' randn_tensor: drawn on the
        generator's device and moved)."""
        import torch
        dev = self.moments.device
        gdev = generator.device if generator is not None else dev
        eps = torch.randn(self.mean.shape, generator=generator, device=gdev, dtype=torch.float32).to(dev).contiguous()
        B, _, h, w = self.mean.shape
        out = torch.empty(B, 4, h, w, device=dev)
        for b in range(B):
            self.encoder._chk(self.encoder.lib.rt_vae_posterior_sample(self.encoder.h, _ptr(self.moments[b]), _ptr(eps[b]), h, w,
                                                                       C.c_float(float(scale)), _ptr(out[b])))
        return out


class EncoderOutput:
    def __init__(self, latent_dist):
        self.latent_dist = latent_dist
