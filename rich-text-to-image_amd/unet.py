"""`unet(sample, t, encoder_hidden_states, added_cond_kwargs)['sample']` seam
(models/unet_2d_condition.py:703-717) backed by the HIP engine."""
import types

import torch

from .engine import Engine
from .controlnet import ControlNetMixin
from .pag import PagMixin
from .ip_adapter import IPAdapterMixin
from .regional_lora import RegionalLoraMixin, is_wide, rank_layout


class HipUNet2DConditionModel(IPAdapterMixin, ControlNetMixin, RegionalLoraMixin, PagMixin):
    """Holds the engine(s) for one set of weights; engines are created lazily per latent size.  With an IP-Adapter installed
    (load_ip_adapter) every engine is built with its image tokens per prompt and carries its to_k_ip / to_v_ip weights; with a ControlNet installed
    (load_controlnet) every engine is built with it and carries its weights under "controlnet.".  With regional LoRA adapters installed
    (load_regional_loras) every engine is built with their rank columns and carries their factors under "lora.".  The operator seam
    __call__ stays text-only, uncontrolled and un-adapted."""

    def __init__(self, config, state_dict=None, device=0, max_streams=8, max_prompts=8, max_keys=77):
        self.config_dict = dict(config)
        self.config = types.SimpleNamespace(**config)
        self.in_channels = config["in_channels"]
        self.device_index = device
        self.max_streams, self.max_prompts, self.max_keys = max_streams, max_prompts, max_keys
        self._state_dict = state_dict
        self._engines = {}
        self.freeu = None                          # (s1, s2, b1, b2) or None = off: on every engine of this model, present and future
        self.ip_tokens, self._ip_weights = 0, None # install_ip_adapter: image tokens per prompt slot (0 = no adapter) and the adapter's layer weights
        self._cn_config, self._cn_weights = None, None   # install_controlnet: Engine's controlnet= argument (None = no ControlNet) and the ControlNet's weights
        self.lora_rank, self._rl_adapters = 0, None      # install_regional_loras: Engine's lora_rank= argument (0 = none) and the parsed adapters
        self.lora_targets = 0                            # ... and its lora_targets=: 1 when an adapter sits on ff.net.0.proj / ff.net.2 / proj_in / proj_out

    def install_regional_loras(self, adapters):
        """adapters: {name: modules} (regional_lora.parse_adapter) or None = remove them.  As install_ip_adapter: the weight table changes,
        the engines are dropped and rebuilt on their next use, and a model whose weights arrived by broadcast refuses once it has an engine."""
        if isinstance(self._state_dict, str) and self._state_dict == "empty" and self._engines:
            raise RuntimeError("HipUNet2DConditionModel: the weights of this model arrived by broadcast and live in its engines only; "
                               "load / unload regional LoRA adapters before the first engine is built")
        self.lora_rank, self._rl_adapters = (rank_layout(adapters)[3], adapters) if adapters else (0, None)
        self.lora_targets = int(any(is_wide(p) for m in (adapters or {}).values() for p in m))
        for e in self._engines.values():
            e.close()
        self._engines = {}

    def install_controlnet(self, cn):
        """cn: what controlnet.load_controlnet returns, or None = remove it.  As install_ip_adapter: the weight table changes, the engines
        are dropped and rebuilt on their next use, and a model whose weights arrived by broadcast refuses once it has an engine."""
        if isinstance(self._state_dict, str) and self._state_dict == "empty" and self._engines:
            raise RuntimeError("HipUNet2DConditionModel: the weights of this model arrived by broadcast and live in its engines only; "
                               "load / unload a ControlNet before the first engine is built")
        self._cn_config = dict(embed_channels=cn["embed_channels"], hint_channels=cn["hint_channels"]) if cn is not None else None
        self._cn_weights = cn["weights"] if cn is not None else None
        for e in self._engines.values():
            e.close()
        self._engines = {}

    def install_ip_adapter(self, adapter):
        """adapter: what ip_adapter.load_ip_adapter returns, or None = remove it.  The weight table - and with it the arena - changes, so
        the engines are dropped and rebuilt on their next use.  A model built "empty" (ranks != 0 of a multi-GPU launch) holds its weights
        nowhere but in the arena of its engines, which a changed layout could not take over: once it has an engine this is refused and
        nothing changes - install the adapter before the first engine() call, as sample.build_model does."""
        if isinstance(self._state_dict, str) and self._state_dict == "empty" and self._engines:
            raise RuntimeError("HipUNet2DConditionModel: the weights of this model arrived by broadcast and live in its engines only; "
                               "load / unload an IP-Adapter before the first engine is built")
        self.ip_tokens, self._ip_weights = (adapter["T"], adapter["weights"]) if adapter is not None else (0, None)
        for e in self._engines.values():
            e.close()
        self._engines = {}

    def enable_freeu(self, s1, s2, b1, b2):
        """diffusers' `unet.enable_freeu(s1, s2, b1, b2)` (argument order included): FreeU in the first two up blocks of every forward
        of this model (Engine.set_freeu), until disable_freeu()."""
        from .freeu import check_freeu
        self.freeu = check_freeu((s1, s2, b1, b2), "HipUNet2DConditionModel.enable_freeu")
        for e in self._engines.values():
            e.set_freeu(*self.freeu)

    def disable_freeu(self):
        self.freeu = None
        for e in self._engines.values():
            e.disable_freeu()

    def load_state_dict(self, sd):
        self._state_dict = sd
        for e in self._engines.values():
            e.load_state_dict(sd)

    def engine(self, h, w, streams=None, prompts=None, keys=None):
        """Engine for latent size (h, w).  `streams` / `prompts` / `keys`: what the caller is about to use (F batched forwards per step,
        P prompts in the K/V cache, the keys of the longest prompt: 77 per CLIP window); an engine sized for fewer is rebuilt once with
        room for them (<= 16 streams, <= 231 keys).  If the rebuild fails the old engines AND the old limits stay."""
        grow = False
        limits = (self.max_streams, self.max_prompts, self.max_keys)
        # every request is checked before any limit moves: a refused call leaves the limits the engines were built for
        if keys and keys > self.max_keys and keys not in (154, 231):
            raise ValueError(f"{keys} cross-attention keys per prompt: the engine takes 77, 154 or 231 (one to three CLIP windows)")
        if streams and streams > 16:
            raise ValueError(f"{streams} batched UNet forwards per step exceed the engine limit of 16 (at most 13 regions with injection)")
        if keys and keys > self.max_keys:
            self.max_keys, grow = keys, True
        if streams and streams > self.max_streams:
            self.max_streams, grow = min(16, max(streams, 2 * self.max_streams)), True
        if prompts and prompts > self.max_prompts:
            self.max_prompts, grow = max(prompts, 2 * self.max_prompts), True
        empty = isinstance(self._state_dict, str) and self._state_dict == "empty"
        # A model built "empty" (ranks != 0 of a seed-parallel launch) holds weights that exist nowhere else on this rank: the packed
        # arena it received by launcher.broadcast_weights.  Its layout is a function of the config alone (not of the stream / prompt
        # capacity or the latent size), so a new engine - a grown one, or one for another latent size - takes it over device to
        # device from ANY engine that is bound.  The donor stays registered until the copy has succeeded: if the
        # allocation of the new engine fails, nothing is lost.
        donor = next((e for e in self._engines.values() if e.weights_missing()[0] == 0), None) if empty else None
        stale = dict(self._engines) if grow else {}
        if grow:
            self._engines = {}
        key = (h, w)
        if key not in self._engines:
            if self._state_dict is None:
                raise RuntimeError("HipUNet2DConditionModel: no weights loaded (call load_state_dict)")
            try:
                e = Engine(self.config_dict, h, w, device=self.device_index, max_streams=self.max_streams,
                           max_prompts=self.max_prompts, max_keys=self.max_keys, ip_tokens=self.ip_tokens, controlnet=self._cn_config,
                           lora_rank=self.lora_rank, lora_targets=self.lora_targets)
                try:
                    if empty:
                        if donor is not None:
                            from .launcher import arena_tensor
                            src, dst = arena_tensor(donor), arena_tensor(e)
                            if src.numel() != dst.numel():
                                raise RuntimeError(f"weight arena layout changed with the engine capacity ({src.numel()} vs {dst.numel()} bytes)")
                            dst.copy_(src)
                            torch.cuda.synchronize(self.device_index)
                            e.arena_mark_bound()
                        # otherwise the packed arena arrives by launcher.broadcast_weights
                    elif isinstance(self._state_dict, str) and self._state_dict.startswith("random"):
                        e.init_random_weights(seed=int(self._state_dict[6:] or 0))      # "random<seed>": benchmarks without checkpoints
                        for name, t in {**(self._ip_weights or {}), **(self._cn_weights or {})}.items():
                            e.bind_weight(name, t.to(f"cuda:{self.device_index}"))
                        e.synchronize()
                    elif self._ip_weights or self._cn_weights:
                        e.load_state_dict({**self._state_dict, **(self._ip_weights or {}), **(self._cn_weights or {})})
                    else:
                        e.load_state_dict(self._state_dict)
                    if self.lora_rank:                     # (on a broadcast-fed rank the arena that arrives carries the same factors)
                        e.bind_regional_loras(self._rl_adapters)
                    if self.freeu is not None:
                        e.set_freeu(*self.freeu)
                except BaseException:
                    e.close()
                    raise
            except BaseException:
                if grow:                                   # the old engines (and the only copy of a broadcast-fed rank's weights) stay usable,
                    self._engines = stale                  # and so do the limits they were built for: the next call tries the growth again
                    self.max_streams, self.max_prompts, self.max_keys = limits
                raise
            self._engines[key] = e
        for old in stale.values():                         # the rebuilt engine is bound: the smaller ones can go
            old.close()
        return self._engines[key]

    def __call__(self, sample, timestep, encoder_hidden_states, added_cond_kwargs=None, **kw):
        """Batch of independent samples; every sample uses its own row of `encoder_hidden_states`."""
        B, _, h, w = sample.shape
        eng = self.engine(h, w, keys=encoder_hidden_states.shape[1])
        pooled = tid = None
        if added_cond_kwargs is not None:
            pooled, tid = added_cond_kwargs["text_embeds"], added_cond_kwargs["time_ids"][:1]
        eng.set_prompts(encoder_hidden_states, pooled, tid)
        eng.set_fontsize(None, None)
        out = eng.unet_forward(sample, float(timestep), list(range(B)))
        return {"sample": out}
