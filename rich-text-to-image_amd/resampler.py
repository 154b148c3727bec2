"""The Resampler of the IP-Adapter "plus" checkpoints on the engine's operators: a small perceiver in which T <= 16 learned latent queries
attend over the image encoder's penultimate hidden states (and over themselves) and come out as the T image tokens of a prompt slot.
Mirrors clip_vision_encoder.py: bf16 weights, fp32 trunk, every contraction `rt_op_gemm`, LayerNorm `rt_op_layernorm`, GELU
`rt_op_activation`, the attention the kernel of `csrc/resampler.hip` (`rt_op_latent_attention`); torch allocates buffers and copies rows -
no torch arithmetic on the path.

[memory] of the IP-Adapter repository's resampler.py (Resampler.forward, PerceiverAttention, FeedForward):

    x = proj_in(hidden)                                   # Linear(E, dim), bias
    lat = latents.repeat(B)                               # [1, T, dim] parameter
    for each layer:
        xn, ln = norm1(x), norm2(lat)                     # LayerNorm(dim), eps 1e-5
        q = to_q(ln); k, v = to_kv(cat([xn, ln], 1)).chunk(2, -1)     # no biases; inner = heads * dim_head
        lat = to_out(softmax(q k^T dim_head^-1/2) v) + lat            # keys = the N image tokens AND the T latents
        lat = W2 gelu_erf(W1 LayerNorm(lat)) + lat                    # no biases
    return norm_out(proj_out(lat))                        # Linear(dim, D), LayerNorm(D)

Checkpoint keys (under image_proj.): latents, proj_in.{weight,bias}, proj_out.{weight,bias}, norm_out.{weight,bias},
layers.{i}.0.{norm1,norm2}.{weight,bias}, layers.{i}.0.{to_q,to_kv,to_out}.weight, layers.{i}.1.0.{weight,bias} (the feed-forward's
LayerNorm), layers.{i}.1.1.weight, layers.{i}.1.3.weight.  Every dimension is read from the shapes except dim_head (64 in every published
checkpoint).

Limits: T <= 16, dim and D <= 2048, N + T <= 656 keys, dim_head a multiple of 8 and <= 128, every width a multiple of 8.

The GEMMs of a call run image by image (the other operators take the whole batch): an image's tokens do not depend on what else is in
the call, bit for bit, whatever tile the GEMM picks for another row count."""
import ctypes as C

MAX_TOKENS = 16          # ip_adapter.MAX_TOKENS: one MFMA query tile of rt_op_latent_attention
MAX_KEYS = 656           # the encoder's 640 tokens + 16 latents
MAX_WIDTH = 2048         # rt_op_layernorm
TOP_KEYS = ("latents", "proj_in", "proj_out", "norm_out", "layers")


def is_resampler_key(k):
    """k: a key below image_proj."""
    return k.split(".")[0] in TOP_KEYS


def layer_shapes(i, dim, inner, ff):
    p = f"layers.{i}."
    return {p + "0.norm1.weight": (dim,), p + "0.norm1.bias": (dim,), p + "0.norm2.weight": (dim,), p + "0.norm2.bias": (dim,),
            p + "0.to_q.weight": (inner, dim), p + "0.to_kv.weight": (2 * inner, dim), p + "0.to_out.weight": (dim, inner),
            p + "1.0.weight": (dim,), p + "1.0.bias": (dim,), p + "1.1.weight": (ff, dim), p + "1.3.weight": (dim, ff)}


def check_resampler(proj, dim_head=64, who="IP-Adapter"):
    """The tensors below image_proj. of a plus checkpoint -> dict(weights = {key: fp32 host tensor}, E, dim, D, T, depth, heads, dim_head,
    inner, ff).  ValueError naming the key for a missing, left-over or mis-shaped tensor and for inner % dim_head.  No GPU needed."""
    def need(k, dims=None):
        if k not in proj:
            raise ValueError(f"{who}: missing key image_proj.{k}")
        if dims is not None and proj[k].dim() != dims:
            raise ValueError(f"{who}: image_proj.{k} has shape {tuple(proj[k].shape)}, expected {dims} dimensions")
        return tuple(int(s) for s in proj[k].shape)
    lt = need("latents", 3)
    if lt[0] != 1 or not 1 <= lt[1] <= MAX_TOKENS:
        raise ValueError(f"{who}: image_proj.latents has shape {lt}, expected [1, T, dim] with T in 1 .. {MAX_TOKENS}")
    T, dim = lt[1], lt[2]
    E = need("proj_in.weight", 2)[1]
    D = need("proj_out.weight", 2)[0]
    need("layers.0.0.to_q.weight", 2)
    inner = need("layers.0.0.to_q.weight")[0]
    ff = need("layers.0.1.1.weight", 2)[0]
    depth = 1 + max(int(k.split(".")[1]) for k in proj if k.startswith("layers.") and k.split(".")[1].isdigit())
    if not isinstance(dim_head, int) or dim_head <= 0 or dim_head % 8 or dim_head > 128:
        raise ValueError(f"{who}: dim_head must be a multiple of 8 in 8 .. 128, got {dim_head!r}")
    if inner % dim_head:
        raise ValueError(f"{who}: image_proj.layers.0.0.to_q.weight has {inner} rows (inner = heads * dim_head): not a multiple of dim_head = {dim_head}")
    want = {"latents": (1, T, dim), "proj_in.weight": (dim, E), "proj_in.bias": (dim,), "proj_out.weight": (D, dim), "proj_out.bias": (D,),
            "norm_out.weight": (D,), "norm_out.bias": (D,)}
    for i in range(depth):
        want.update(layer_shapes(i, dim, inner, ff))
    for k, shape in want.items():
        if k not in proj:
            raise ValueError(f"{who}: missing key image_proj.{k}")
        if tuple(proj[k].shape) != shape:
            raise ValueError(f"{who}: image_proj.{k} has shape {tuple(proj[k].shape)}, expected {shape}")
    left = sorted(set(proj) - set(want))
    if left:
        raise ValueError(f"{who}: left-over key image_proj.{left[0]} ({len(left)} in all): not a tensor of the Resampler")
    for name, val in (("embedding_dim (image_proj.proj_in.weight columns)", E), ("dim (image_proj.latents)", dim),
                      ("the output width (image_proj.proj_out.weight rows)", D), ("the feed-forward width (image_proj.layers.0.1.1.weight rows)", ff)):
        if val % 8:
            raise ValueError(f"{who}: {name} must be a multiple of 8, got {val}")
    if dim > MAX_WIDTH or D > MAX_WIDTH:
        raise ValueError(f"{who}: image_proj.latents / image_proj.proj_out.weight: dim and the output width must be <= {MAX_WIDTH}, got {dim} / {D}")
    return dict(weights={k: proj[k].detach().float() for k in want}, E=E, dim=dim, D=D, T=T, depth=depth, heads=inner // dim_head,
                dim_head=dim_head, inner=inner, ff=ff)


def _ptr(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


class HipResampler:
    """`resampler`: check_resampler's result (load_ip_adapter(...)["resampler"]).  __call__(hidden [B, N, E] fp32) -> [B, T, D] fp32 on
    the GPU (the values are bf16-rounded by the last LayerNorm, like ip_adapter.project's)."""

    def __init__(self, resampler, device=0):
        import torch
        from .engine import load_library
        r = resampler
        self.E, self.dim, self.D, self.T, self.depth = r["E"], r["dim"], r["D"], r["T"], r["depth"]
        self.heads, self.dim_head, self.inner, self.ff = r["heads"], r["dim_head"], r["inner"], r["ff"]
        self.eps = 1e-5
        self.lib = load_library()
        self.device = device
        self.dev = torch.device(f"cuda:{device}")
        w = r["weights"]
        f32 = lambda k: w[k].float().to(self.dev).contiguous()
        b16 = lambda k: w[k].float().to(torch.bfloat16).to(self.dev).contiguous()
        self.latents = f32("latents").reshape(self.T, self.dim)
        self.w_in, self.b_in = b16("proj_in.weight"), f32("proj_in.bias")
        self.w_out, self.b_out = b16("proj_out.weight"), f32("proj_out.bias")
        self.norm_out = (f32("norm_out.weight"), f32("norm_out.bias"))
        self.layers = []
        for i in range(self.depth):
            p = f"layers.{i}."
            self.layers.append(dict(n1=(f32(p + "0.norm1.weight"), f32(p + "0.norm1.bias")), n2=(f32(p + "0.norm2.weight"), f32(p + "0.norm2.bias")),
                                    wq=b16(p + "0.to_q.weight"), wkv=b16(p + "0.to_kv.weight"), wo=b16(p + "0.to_out.weight"),
                                    nf=(f32(p + "1.0.weight"), f32(p + "1.0.bias")), w1=b16(p + "1.1.weight"), w2=b16(p + "1.3.weight")))

    def parameter_tensors(self):
        """Every device-resident weight in a fixed order."""
        out = [self.latents, self.w_in, self.b_in]
        for ly in self.layers:
            out += [ly["n1"][0], ly["n1"][1], ly["n2"][0], ly["n2"][1], ly["wq"], ly["wkv"], ly["wo"], ly["nf"][0], ly["nf"][1], ly["w1"], ly["w2"]]
        return out + [self.w_out, self.b_out, self.norm_out[0], self.norm_out[1]]

    def _chk(self, rc):
        if rc != 0:
            from .engine import RtError
            raise RtError(rc, self.lib.rt_op_last_error().decode())

    def _gemm(self, A, W, bias, out, rows, epi=0, res=None):
        """out = A W^T (+ bias) (+ res), one launch per image of `rows` rows each (see the module docstring)."""
        K, N = A.shape[1], W.shape[0]
        for r0 in range(0, A.shape[0], rows):
            a, o = A[r0:r0 + rows], out[r0:r0 + rows]
            rs = res[r0:r0 + rows] if res is not None else None
            self._chk(self.lib.rt_op_gemm(_ptr(a), _ptr(W), _ptr(bias), _ptr(o), _ptr(rs), None, 0, epi, rows, N, K, A.stride(0), W.stride(0),
                                          out.stride(0), res.stride(0) if res is not None else 0, 0, 0, 0, 0, 0, 0, 0, None))

    def _ln(self, x, wb, out, rows=None):
        """LayerNorm of the dense fp32 rows x -> the dense bf16 rows at `out` (a tensor whose first rows are written)."""
        self._chk(self.lib.rt_op_layernorm(_ptr(x), _ptr(wb[0]), _ptr(wb[1]), _ptr(out), x.shape[0] if rows is None else rows, x.shape[1],
                                           C.c_float(self.eps), None))

    def __call__(self, hidden):
        import torch
        h = torch.as_tensor(hidden)
        if h.dim() != 3 or h.shape[2] != self.E or h.shape[0] < 1 or h.shape[1] < 1:
            raise ValueError(f"hidden states must be [B, N, {self.E}], got {tuple(h.shape)}")
        B, N = int(h.shape[0]), int(h.shape[1])
        T, dim, inner, Nk = self.T, self.dim, self.inner, N + self.T
        if Nk > MAX_KEYS:
            raise ValueError(f"{N} hidden states + {T} latents = {Nk} keys: at most {MAX_KEYS}")
        bf = torch.bfloat16
        with torch.cuda.device(self.dev):
            h = h.detach().to(self.dev, torch.float32).reshape(B * N, self.E).contiguous()
            new = lambda rows, cols, dt=bf: torch.empty(rows, cols, device=self.dev, dtype=dt)
            hb = new(B * N, self.E)
            self._chk(self.lib.rt_op_cast_bf16(_ptr(h), _ptr(hb), C.c_longlong(h.numel()), None))
            x = new(B * N, dim, torch.float32)
            self._gemm(hb, self.w_in, self.b_in, x, N, epi=1)
            lat = self.latents.repeat(B, 1).contiguous()                            # fp32 trunk [B T, dim]
            xl, lnq = new(B * Nk, dim), new(B * T, dim)                             # per image [xn; ln], and ln alone for to_q
            kv, q, att = new(B * Nk, 2 * inner), new(B * T, inner), new(B * T, inner)
            hf, f1, f2 = new(B * T, dim), new(B * T, self.ff), new(B * T, self.ff)
            for ly in self.layers:
                for b in range(B):                                                  # norm1(x) of image b -> the first N rows of its block
                    self._ln(x[b * N:(b + 1) * N], ly["n1"], xl[b * Nk:])
                self._ln(lat, ly["n2"], lnq)
                xl.view(B, Nk, dim)[:, N:].copy_(lnq.view(B, T, dim))               # plain copy: the T latent rows behind them
                self._gemm(lnq, ly["wq"], None, q, T)
                self._gemm(xl, ly["wkv"], None, kv, Nk)
                self._chk(self.lib.rt_op_latent_attention(_ptr(q), inner, _ptr(kv), _ptr(kv, 2 * inner), 2 * inner, _ptr(att), inner, B, self.heads,
                                                          T, Nk, self.dim_head, C.c_float(self.dim_head ** -0.5), None))
                self._gemm(att, ly["wo"], None, lat, T, epi=1, res=lat)
                self._ln(lat, ly["nf"], hf)
                self._gemm(hf, ly["w1"], None, f1, T)
                self._chk(self.lib.rt_op_activation(_ptr(f1), _ptr(f2), C.c_longlong(f1.numel()), 1, None))
                self._gemm(f2, ly["w2"], None, lat, T, epi=1, res=lat)
            lb = new(B * T, dim)
            self._chk(self.lib.rt_op_cast_bf16(_ptr(lat), _ptr(lb), C.c_longlong(lat.numel()), None))
            y = new(B * T, self.D, torch.float32)
            self._gemm(lb, self.w_out, self.b_out, y, T, epi=1)
            out = new(B * T, self.D)
            self._ln(y, self.norm_out, out)
            torch.cuda.synchronize(self.dev)
        return out.float().reshape(B, T, self.D)


class LazyResampler:
    """check_resampler's result kept on the host; the device object is built with the first picture, on the device that uses it."""
    def __init__(self, resampler):
        self.host = resampler
        self._dev = {}

    def on(self, device):
        if device not in self._dev:
            self._dev[device] = HipResampler(self.host, device=device)
        return self._dev[device]
