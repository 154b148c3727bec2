"""Thin torch<->C-ABI helpers for the GPU parity tests (call the product kernels through include/rtdiff.h)."""
import ctypes as C

import torch

from rich_text_to_image_amd.engine import load_library, _ptr

DEV = "cuda:0"


def blank(*shape, dtype=torch.float32):
    """An output buffer pre-filled with NaN (torch.empty hands back a cached block that may still hold the previous launch's correct
    values): an element a kernel never writes fails the comparison that follows."""
    return torch.full(shape, float("nan"), device=DEV, dtype=dtype)


def chk(rc):
    if rc != 0:
        raise RuntimeError(f"rt_op error {rc}: {load_library().rt_op_last_error().decode()}")


def bf(t):
    return t.to(DEV).to(torch.bfloat16).contiguous()


def gemm(A, W, bias=None, epi=0, res=None, temb=None, rows_per_batch=0, mode=0, conv=None, out_cols=None, out=None):
    """A: bf16 [M,K] (dense) or NHWC [B,Hin,Win,Cin] (conv); W bf16 [N,K].  Leading dimensions are the operands' own row strides (A, W,
    res, temb may be windows of wider buffers); out: the caller's [M, columns] window instead of a fresh exact allocation."""
    lib = load_library()
    N, K = W.shape
    if mode == 0:
        M = A.shape[0]
        Hin = Win = Cin = Hout = Wout = 0
        lda = A.stride(0)
    else:
        B, Hin, Win, Cin = A.shape
        Hout, Wout = conv
        M = B * Hout * Wout
        rows_per_batch = Hout * Wout
        lda = 0
    oc = out_cols if out_cols is not None else (N // 2 if epi == 3 else N)
    odt = {1: torch.float32, 4: torch.float16}.get(epi, torch.bfloat16)
    if out is None:
        out = blank(M, oc, dtype=odt)
    assert out.shape == (M, oc) and out.dtype == odt and out.stride(1) == 1
    chk(lib.rt_op_gemm(_ptr(A), _ptr(W), _ptr(bias), _ptr(out), _ptr(res), _ptr(temb), mode, epi, M, N, K, lda, W.stride(0),
                       out.stride(0), res.stride(0) if res is not None else 0, temb.stride(0) if temb is not None else 0,
                       rows_per_batch, Hin, Win, Cin, Hout, Wout, None))
    torch.cuda.synchronize()
    return out


def attention(Q, K, VT, B, H, N, NK, DP, ldq=None, ldk=None, q_src=None, k_src=None, v_src=None, cross=False, wabs=None,
              wsgn=None, wset=None, nk_valid=None, O=None):
    """O: the caller's [B*N, H*DP] window instead of a fresh exact allocation; V^T's leading dimension is VT's own row stride."""
    lib = load_library()
    if O is None:
        O = blank(B * N, H * DP, dtype=torch.bfloat16)
    assert O.shape == (B * N, H * DP) and O.dtype == torch.bfloat16 and O.stride(1) == 1

    def ia(v):
        return (C.c_int * B)(*v) if v is not None else None
    chk(lib.rt_op_attention(_ptr(Q), ldq or Q.stride(0), _ptr(K), ldk or K.stride(0), _ptr(VT), VT.stride(0), _ptr(O), O.stride(0),
                            ia(q_src), ia(k_src), ia(v_src), ia(wset), _ptr(wabs), _ptr(wsgn), B, H, N, NK,
                            nk_valid if nk_valid is not None else NK, DP, int(cross), None))
    torch.cuda.synchronize()
    return O


def groupnorm(x1, x2, G, gamma, beta, eps, silu, want_raw=False):
    lib = load_library()
    in_bf16 = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[x1.dtype]
    B, HW, C1 = x1.shape
    C2 = x2.shape[2] if x2 is not None else 0
    out = blank(B, HW, C1 + C2, dtype=torch.bfloat16)
    raw = blank(B, HW, C1 + C2, dtype=torch.bfloat16) if want_raw else None
    chk(lib.rt_op_groupnorm(_ptr(x1), _ptr(x2), int(in_bf16), C1, C2, G, B, HW, _ptr(gamma), _ptr(beta), C.c_float(eps),
                            int(silu), _ptr(out), _ptr(raw), None))
    torch.cuda.synchronize()
    return (out, raw) if want_raw else out


def layernorm(x, gamma, beta, eps=1e-5):
    lib = load_library()
    rows, Cc = x.shape
    out = blank(rows, Cc, dtype=torch.bfloat16)
    fn = lib.rt_op_layernorm_f16 if x.dtype == torch.float16 else lib.rt_op_layernorm
    chk(fn(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(out), rows, Cc, C.c_float(eps), None))
    torch.cuda.synchronize()
    return out


def small_linear(a, W, bias, silu_in=False, out=None, accumulate=False):
    """out: the caller's [B, N] fp32 window (accumulate: out += ...) instead of a fresh exact allocation."""
    lib = load_library()
    B, K = a.shape
    N = W.shape[0]
    if out is None:
        assert not accumulate
        out = blank(B, N)
    assert out.shape == (B, N) and out.dtype == torch.float32 and out.stride(1) == 1
    chk(lib.rt_op_small_linear(_ptr(a), a.stride(0), _ptr(W), W.stride(0), _ptr(bias), _ptr(out), out.stride(0), B, N, K, int(silu_in),
                               int(accumulate), None))
    torch.cuda.synchronize()
    return out


def timestep_embed(t, dim):
    lib = load_library()
    out = blank(t.numel(), dim)
    chk(lib.rt_op_timestep_embed(_ptr(t), t.numel(), dim, _ptr(out), dim, None))
    torch.cuda.synchronize()
    return out


def report(name, got, ref, atol, rtol):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    bad = err > tol
    msg = (f"{name}: max|err|={err.max().item():.4e} at {tuple(int(v) for v in torch.nonzero(err == err.max())[0])} "
           f"ref_rms={ref.pow(2).mean().sqrt().item():.4e} rel_l2={(err.pow(2).sum() / ref.pow(2).sum().clamp_min(1e-30)).sqrt().item():.4e} "
           f"bad={int(bad.sum())}/{bad.numel()}")
    print(msg)
    assert not bad.any(), msg


def probs_avg_rc(Q, K, out, H, N, NK, NKpad, NKrows, DP, accumulate=0, q_row0=0, k_row0=0):
    """rt_op_attention_probs_avg on the caller's buffers (`out` may be a view into a guard-banded allocation); returns the error code."""
    lib = load_library()
    rc = lib.rt_op_attention_probs_avg(_ptr(Q), Q.stride(0), C.c_longlong(q_row0), _ptr(K), K.stride(0), C.c_longlong(k_row0), _ptr(out),
                                       H, N, NK, NKpad, NKrows, DP, int(accumulate), None)
    torch.cuda.synchronize()
    return rc


def cross_route(C_, heads, d, DP, tokens, prompt_rows, key_counts, folded=False, recorded=False, lib=None):
    """rt_op_cross_route (host only, under the current switches): (kind, hand-over, [kernel of every stream]) of the forward's attn2 launch."""
    B = len(key_counts)
    kind, hand, kern = C.c_int(-9), C.c_int(-9), (C.c_int * B)(*([-9] * B))
    chk((lib or load_library()).rt_op_cross_route(C_, heads, d, DP, tokens, prompt_rows, (C.c_int * B)(*key_counts), B, int(folded), int(recorded),
                                                  C.byref(kind), C.byref(hand), kern))
    return kind.value, hand.value, list(kern)


def store_handover(Q, K, VT, O, out, B, H, N, NK, d, DP, store_stream, cross=False, qk_src=None, prompt=None, key_counts=None, accumulate=0):
    """rt_op_attention_store_handover: the attention launch (writes O) + the store of `store_stream` (writes out); True when the
    attention launch handed its softmax statistics to the store."""
    lib = load_library()

    def ia(v):
        return (C.c_int * B)(*v) if v is not None else None
    taken = C.c_int(-1)
    chk(lib.rt_op_attention_store_handover(_ptr(Q), Q.stride(0), _ptr(K), K.stride(0), _ptr(VT), VT.stride(0), _ptr(O), O.stride(0),
                                           ia(qk_src), ia(prompt), ia(key_counts), None, None, B, H, N, NK, d, DP, int(cross),
                                           store_stream, _ptr(out), int(accumulate), C.byref(taken), None))
    torch.cuda.synchronize()
    assert taken.value in (0, 1)
    return bool(taken.value)
