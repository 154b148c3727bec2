"""The VAE's kernels one call at a time (rt_op_gemm_hilo, rt_op_split_bf16, rt_op_vae_groupnorm[_bwd], rt_op_softmax_rows / _bwd,
rt_op_transpose_bf16, rt_op_sumpool2x2, rt_op_pq_conv_*, rt_op_color_loss_grad): the entries issue the launches of rt_vae from the
same argument builders (csrc/vae.h).  Inside rt_vae every buffer is a slice of one bump-allocated workspace whose neighbours are live
tensors, and the end-to-end tests see one relative L2 over a whole decode; here every case runs

  1. the memory contract of tests/memguard.py FIRST (as tests/test_memory_contract_gpu.py): outputs are guard-banded NaN-filled windows -
     with a padded ldo where the entry takes one - inputs NaN-poisoned outside their extent (padded lda / ldw / ldres), guards intact,
     window fully written;
  2. the plain run on exact allocations, equal to the contract run bit for bit;
  3. the fp64 reference of tests/vae_ops_ref.py on the operands the kernel read, at the bar stated there: derived where it can be
     (bit equality, 2^-8 / 2^-16 of a bf16 plane / pair, 2^-22 / 2^-21 sum bounds), else 8 x the error measured on the MI355X
     (profiles/vae_ops_parity.txt).  Every figure is printed before it is asserted ("FIGURE <bar> <case> <value>").

tests/test_vae_ops_ref.py proves on the CPU, for these inputs, that the emulated faults (a dropped or doubled lo pass, a missing mean
term of GroupNorm backward, a dropped row dot, the open clamp interval, ...) exceed those bars by >= 10 x.  Shapes are the smallest that
take each branch (tests/memcases.py HILO_CASES with their routes - checked on the CPU by tests/test_gemm_route.py; the GroupNorm /
softmax / pool / colour cases of vae_ops_ref.py)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import vae_ops_ref as R  # noqa: E402
from hiputil import DEV, chk, report  # noqa: E402
from memcases import HILO_CASES, KIND_NAMES, TRIPLE, hilo_id, hilo_route_args  # noqa: E402
from memguard import damage, guarded, intact, poisoned  # noqa: E402
from test_memory_contract_gpu import F32_OUT, PAD, _lib, _ptr, check_equal, check_windows, nans, out_window, pz, switches  # noqa: E402

F = C.c_float


def judge(key, name, value):
    print(f"FIGURE {key} {name} {value:.4e} (bar {R.bar(key):.3e})")
    assert value <= R.bar(key), f"{name}: {key} error {value:.4e} above the bar {R.bar(key):.3e}"


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(name, got, want):
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    bad = bits(got) != bits(want)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {bad.numel()} elements differ in bits, first at {tuple(int(v) for v in torch.nonzero(bad)[0])}"


def flat_window(shape, dtype):
    """A guard-banded NaN window for an output without a leading dimension (rows x last dim, ld = last dim)."""
    rows = 1
    for s in shape[:-1]:
        rows *= s
    return guarded((rows, shape[-1]), dtype, device=DEV)


def bounded(name, got, ref, tol):
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    over = err > tol
    print(f"{name}: max |err| / tol = {(err / tol.clamp_min(1e-300)).max().item():.3f}")
    assert bool(torch.isfinite(got).all()) and not bool(over.any()), f"{name}: {int(over.sum())} of {over.numel()} elements outside the derived bound"


# ----------------------------------------------------------------------------------------------- rt_op_gemm_hilo: every route of the contraction
def _hilo(c, A, W, bias, res, out, pair_lo=None, hilo=True):
    M, N, K, Ho, Wo = R.hilo_shape(c)
    conv = c["mode"] != 0
    rc = _lib().rt_op_gemm_hilo(_ptr(A[0]), _ptr(A[1] if hilo else None), _ptr(W[0]), _ptr(W[1] if hilo else None), _ptr(bias), _ptr(out), _ptr(pair_lo),
                                _ptr(res), c["mode"], M, N, K, 0 if conv else A[0].stride(0), W[0].stride(0), out.stride(0),
                                res.stride(0) if res is not None else 0, Ho * Wo, c.get("H", 0), c.get("W", 0), c.get("Cin", 0), Ho, Wo, None)
    chk(rc)
    torch.cuda.synchronize()
    return out


def _hilo_route(c, pad, hilo=True):
    o = [C.c_int(-9) for _ in range(5)]
    assert _lib().rt_op_gemm_hilo_route(*hilo_route_args(c, pad, hilo), *[C.byref(x) for x in o]) == 0
    return tuple(x.value for x in o)


def _hilo_pair(c, Ad, Wd, bias, res, contract):
    """(out_f32 | hi, lo | None) of one call; contract: guarded windows and poisoned operands, checked before returning."""
    M, N, _, _, _ = R.hilo_shape(c)
    name = hilo_id(c)
    if not contract:
        if c["pair"]:
            hi, lo = nans(M, N, torch.bfloat16), nans(M, N, torch.bfloat16)
            _hilo(c, Ad, Wd, bias, res, hi, lo)
            return hi, lo
        out = res.clone() if c["res"] == "inplace" else nans(M, N)
        return _hilo(c, Ad, Wd, bias, out if c["res"] == "inplace" else res, out), None
    # both planes of an operand share its leading dimension
    Ap, Wp = tuple(pz(t) for t in Ad), tuple(pz(t) for t in Wd)
    if c["pair"]:
        (bh, hi), (bl, lo) = out_window(M, N, torch.bfloat16), out_window(M, N, torch.bfloat16)
        _hilo(c, Ap, Wp, pz(bias), pz(res, N + 4) if res is not None else None, hi, lo)
        check_windows(name, [("hi", bh, hi), ("lo", bl, lo)])
        return hi, lo
    big, win = out_window(M, N, torch.float32, pad=4)
    if c["res"] == "inplace":
        win.copy_(res)                                             # out == res: the window holds the residual, ldres = ldo
        _hilo(c, Ap, Wp, pz(bias), win, win)
    else:
        _hilo(c, Ap, Wp, pz(bias), pz(res, N + 4) if res is not None else None, win)
    check_windows(name, [("out", big, win)])
    return win, None


@pytest.mark.parametrize("case", HILO_CASES, ids=hilo_id)
def test_hilo_contraction(case):
    c, name = case, hilo_id(case)
    M, N, K, _, _ = R.hilo_shape(c)
    A, W, bias, res = R.hilo_inputs(c)
    Ad, Wd, bias, res = tuple(dev(t) for t in A), tuple(dev(t) for t in W), dev(bias), dev(res)
    ref = R.t3(c, Ad, Wd, bias, res)
    with switches(-1, c["debug"]):
        ra, rb = _hilo_route(c, 0), _hilo_route(c, PAD)
        assert ra == rb and (ra[0], ra[3]) == (c["kind"], c["pass_kind"]), f"{name}: takes {KIND_NAMES[ra[0]]} over {KIND_NAMES[ra[3]]}"
        w0, w1 = _hilo_pair(c, Ad, Wd, bias, res, contract=True)
        p0, p1 = _hilo_pair(c, Ad, Wd, bias, res, contract=False)
        check_equal(name, [("out", w0, p0)] + ([("lo", w1, p1)] if c["pair"] else []))
        if c["pair"]:
            # the pair is the split of the fp32 result of the same route: hi == bf16(o), lo == bf16(o - hi), bit for bit
            o = _hilo(dict(c, pair=False), Ad, Wd, bias, res, nans(M, N))
            hi, lo = o.to(torch.bfloat16), (o - o.to(torch.bfloat16).float()).to(torch.bfloat16)
            same_bits(name + " hi", p0, hi)
            same_bits(name + " lo", p1, lo)
            p0 = o
    judge("contraction", name, R.max_over_rms(p0, ref))
    if c["debug"]:
        # the one-launch form of the same problem against the three launches, at the same bar
        fused = _hilo_pair(dict(c, debug=0), Ad, Wd, bias, res, contract=False)[0]
        assert _hilo_route(c, 0)[0] != TRIPLE
        judge("contraction", name + " fused vs three launches", R.max_over_rms(fused, p0))
    else:
        # A_lo == NULL: the single-pass call as the default mode issues it, at the bar of the other fp32-output GEMM tests
        assert _hilo_route(c, 0, hilo=False)[0] == c["pass_kind"]
        inplace = c["res"] == "inplace"
        one = res.clone() if inplace else nans(M, N)
        _hilo(dict(c, pair=False), Ad, Wd, bias, one if inplace else res, one, hilo=False)
        ref1 = R.t3(c, Ad, Wd, bias, res, single=True)
        print(f"FIGURE single_pass {name} {R.max_over_rms(one, ref1):.4e} (measured before: {R.SINGLE_PASS_MEASURED:.3e})")
        report(name + " single pass", one, ref1, **F32_OUT)


# ----------------------------------------------------------------------------------------------- rt_op_split_bf16
@pytest.mark.parametrize("n", R.SPLIT_SIZES)
def test_split_bf16(n):
    x = dev(R.split_values(n))
    (bh, hi), (bl, lo) = guarded((n // 4, 4), torch.bfloat16, device=DEV), guarded((n // 4, 4), torch.bfloat16, device=DEV)

    def run(x_, hi_, lo_):
        chk(_lib().rt_op_split_bf16(_ptr(x_), _ptr(hi_), _ptr(lo_), C.c_longlong(n), None))
        torch.cuda.synchronize()
    run(poisoned(x), hi, lo)
    check_windows(f"split {n}", [("hi", bh, hi), ("lo", bl, lo)])
    ph, pl = nans(n // 4, 4, torch.bfloat16), nans(n // 4, 4, torch.bfloat16)
    run(x, ph, pl)
    check_equal(f"split {n}", [("hi", hi, ph), ("lo", lo, pl)])
    wh, wl = R.split(x)
    same_bits(f"split {n} hi", ph.reshape(-1), wh)
    same_bits(f"split {n} lo", pl.reshape(-1), wl)


# ----------------------------------------------------------------------------------------------- GroupNorm forward (low planes) and backward
GN_RUNS = list(zip(R.GN_CASES, R.GN_VARIANTS))


def _gn_fwd(x, Cc, G, B, HW, gamma, beta, silu, out, out_lo, raw, raw_lo, stats):
    chk(_lib().rt_op_vae_groupnorm(_ptr(x), int(x.dtype == torch.bfloat16), Cc, G, B, HW, _ptr(gamma), _ptr(beta), F(R.GN_EPS), int(silu), _ptr(out),
                                   _ptr(out_lo), _ptr(raw), _ptr(raw_lo), _ptr(stats), None))
    torch.cuda.synchronize()


def _gn_bwd(x, dA, stats, gamma, beta, silu, Cc, G, B, HW, add, out, ob, ol):
    chk(_lib().rt_op_vae_groupnorm_bwd(_ptr(x), int(x.dtype == torch.bfloat16), _ptr(dA[0]), _ptr(dA[1]), _ptr(stats), _ptr(gamma), _ptr(beta), F(R.GN_EPS),
                                       int(silu), Cc, G, B, HW, _ptr(add), _ptr(out), _ptr(ob), _ptr(ol), None))
    torch.cuda.synchronize()


@pytest.mark.parametrize("case,v", GN_RUNS, ids=[R.gn_id(c, v) for c, v in GN_RUNS])
def test_vae_groupnorm_forward_and_backward(case, v):
    Cc, G, HW, B = case
    name = R.gn_id(case, v)
    x, gamma, beta, dA, add = R.gn_inputs(case, v)
    xd = dev(x.to(torch.bfloat16) if v["x_bf16"] else x).reshape(B * HW, Cc)
    gamma, beta, add = dev(gamma), dev(beta), dev(add.reshape(B * HW, Cc)) if add is not None else None
    dAd = tuple(dev(t.reshape(B * HW, Cc)) if t is not None else None for t in dA)
    nchunk = _lib().rt_op_vae_groupnorm_nchunk(HW)
    assert nchunk == -(-HW // max(16, min(128, HW // 128)))
    lo_planes = not v["x_bf16"]                                       # the precise VAE normalises fp32 maps into pairs; bf16 maps belong to the default mode
    # ---- forward: contract run, plain run, reference
    shp = (B * HW, Cc)
    wins = {k: flat_window(shp, torch.bfloat16) for k in (("out", "out_lo", "raw", "raw_lo") if lo_planes else ("out",))}
    sbig, swin = flat_window((B * nchunk * G, 2), torch.float32)
    w = {k: vw[1] for k, vw in wins.items()}
    _gn_fwd(pz(xd, 0), Cc, G, B, HW, pz(gamma), pz(beta), v["silu"], w["out"], w.get("out_lo"), w.get("raw"), w.get("raw_lo"), swin)
    check_windows(name + " forward", [(k, b, vw) for k, (b, vw) in wins.items()])
    # the statistics buffer: nothing outside it; (mean, rstd) in chunk 0's slots (the other slots hold partial sums, or nothing in the one-launch form)
    assert intact(sbig, swin), f"{name}: stray write around the statistics: {damage(sbig, swin)}"
    assert bool(torch.isfinite(swin.reshape(B, nchunk, G, 2)[:, 0]).all())
    p = {k: nans(*vw.shape, vw.dtype) for k, vw in w.items()}
    pstats = nans(B * nchunk * G, 2)
    _gn_fwd(xd, Cc, G, B, HW, gamma, beta, v["silu"], p["out"], p.get("out_lo"), p.get("raw"), p.get("raw_lo"), pstats)
    check_equal(name + " forward", [(k, w[k], p[k]) for k in w])
    st = pstats.reshape(B, nchunk, G, 2)[:, 0]
    assert torch.equal(st, swin.reshape(B, nchunk, G, 2)[:, 0]), f"{name}: statistics differ between the plain and the contract run"
    y, mean, rstd = R.gn_fwd_ref(xd.reshape(B, HW, Cc), G, gamma, beta, v["silu"])
    got = R.pair64(p["out"], p.get("out_lo")).reshape(B, HW, Cc)
    judge("gn_fwd", name, R.needed_R(got, y, rel=R.PAIR_REL if lo_planes else R.HI_REL))
    if lo_planes:
        rh, rl = R.split(xd)
        same_bits(name + " raw", p["raw"], rh)
        same_bits(name + " raw_lo", p["raw_lo"], rl)
    judge("gn_stats", name, max(R.needed_R(st[..., 0], mean), R.needed_R(st[..., 1], rstd)))
    # ---- backward, with the statistics the forward left and with the fp64 statistics rounded to fp32 (everything else of the buffer poisoned)
    exact = torch.full((B, nchunk, G, 2), float("nan"), device=DEV)
    exact[:, 0, :, 0], exact[:, 0, :, 1] = mean.float(), rstd.float()
    ref = R.gn_bwd_ref(xd.reshape(B, HW, Cc), R.pair64(*dAd).reshape(B, HW, Cc), G, gamma, beta, v["silu"], add.reshape(B, HW, Cc) if add is not None else None)
    ref = ref.reshape(B * HW, Cc)
    for key, stats in (("gn_bwd", pstats), ("gn_bwd_exact", exact.reshape(B * nchunk * G, 2))):
        bw = {"ob": flat_window(shp, torch.bfloat16)}
        if v["out"]:
            bw["out"] = flat_window(shp, torch.float32)
        if v["out_lo"]:
            bw["ol"] = flat_window(shp, torch.bfloat16)
        ww = {k: vw[1] for k, vw in bw.items()}
        _gn_bwd(pz(xd, 0), tuple(pz(t, 0) for t in dAd), poisoned(stats), pz(gamma), pz(beta), v["silu"], Cc, G, B, HW, pz(add, 0), ww.get("out"), ww["ob"], ww.get("ol"))
        check_windows(f"{name} {key}", [(k, b, vw) for k, (b, vw) in bw.items()])
        pp = {k: nans(*vw.shape, vw.dtype) for k, vw in ww.items()}
        _gn_bwd(xd, dAd, stats, gamma, beta, v["silu"], Cc, G, B, HW, add, pp.get("out"), pp["ob"], pp.get("ol"))
        check_equal(f"{name} {key}", [(k, ww[k], pp[k]) for k in ww])
        if v["out"]:
            judge(key, name + " out", R.needed_R(pp["out"], ref))
            hi, lo = R.split(pp["out"])                                # the planes are the split of the fp32 result, bit for bit
            same_bits(f"{name} {key} out_bf16", pp["ob"], hi)
            if v["out_lo"]:
                same_bits(f"{name} {key} out_bf16_lo", pp["ol"], lo)
        else:
            judge(key, name + " planes", R.needed_R(R.pair64(pp["ob"], pp.get("ol")), ref, rel=R.PAIR_REL if v["out_lo"] else R.HI_REL))


# ----------------------------------------------------------------------------------------------- softmax forward / backward
@pytest.mark.parametrize("with_lo", [True, False], ids=["pair", "hi"])
@pytest.mark.parametrize("rows,cols", R.SOFTMAX_CASES)
def test_softmax_rows_and_backward(rows, cols, with_lo):
    name = f"softmax {rows}x{cols} lo={with_lo}"
    rel = R.PAIR_REL if with_lo else R.HI_REL
    lib = _lib()
    s = dev(R.softmax_scores(rows, cols))
    wins = {k: flat_window((rows, cols), torch.bfloat16) for k in (("p", "p_lo") if with_lo else ("p",))}
    w = {k: vw[1] for k, vw in wins.items()}

    def fwd(s_, p_, l_):
        chk(lib.rt_op_softmax_rows(_ptr(s_), _ptr(p_), _ptr(l_), rows, cols, F(R.SOFTMAX_SCALE), None))
        torch.cuda.synchronize()
    fwd(pz(s, 0), w["p"], w.get("p_lo"))
    check_windows(name, [(k, b, vw) for k, (b, vw) in wins.items()])
    p = {k: nans(rows, cols, torch.bfloat16) for k in w}
    fwd(s, p["p"], p.get("p_lo"))
    check_equal(name, [(k, w[k], p[k]) for k in w])
    ref = R.softmax_ref(s)
    got = R.pair64(p["p"], p.get("p_lo"))
    judge("softmax", name, R.needed_R(got, ref, rel=rel))
    # row sums: sum |err_i| <= sum (rel p_i + R (rms + p_i)) <= rel + R (sqrt(cols) + 1), since sum p_i^2 <= 1
    rs = (got.sum(-1) - 1).abs().max().item()
    print(f"{name}: max |row sum - 1| = {rs:.3e}")
    assert rs <= rel + R.bar("softmax") * (cols ** 0.5 + 1)
    # ---- backward
    P, dp = R.softmax_bwd_inputs(rows, cols, with_lo)
    P, dp = tuple(dev(t) for t in P), dev(dp)
    bwins = {k: flat_window((rows, cols), torch.bfloat16) for k in (("ds", "ds_lo") if with_lo else ("ds",))}
    bw = {k: vw[1] for k, vw in bwins.items()}

    def bwd(P_, dp_, d_, l_):
        chk(lib.rt_op_softmax_bwd(_ptr(P_[0]), _ptr(P_[1]), _ptr(dp_), _ptr(d_), _ptr(l_), rows, cols, F(R.SOFTMAX_SCALE), None))
        torch.cuda.synchronize()
    bwd(tuple(pz(t, 0) for t in P), pz(dp, 0), bw["ds"], bw.get("ds_lo"))
    check_windows(name + " bwd", [(k, b, vw) for k, (b, vw) in bwins.items()])
    q = {k: nans(rows, cols, torch.bfloat16) for k in bw}
    bwd(P, dp, q["ds"], q.get("ds_lo"))
    check_equal(name + " bwd", [(k, bw[k], q[k]) for k in bw])
    judge("softmax_bwd", name, R.needed_R(R.pair64(q["ds"], q.get("ds_lo")), R.softmax_bwd_ref(P, dp), rel=rel))


# ----------------------------------------------------------------------------------------------- transpose, sum-pool
@pytest.mark.parametrize("rows,cols", R.TRANSPOSE_CASES)
def test_transpose_bf16(rows, cols):
    x = dev(torch.randn(rows, cols, generator=R.gen(rows + cols)).to(torch.bfloat16))
    big, win = flat_window((cols, rows), torch.bfloat16)

    def run(x_, o_):
        chk(_lib().rt_op_transpose_bf16(_ptr(x_), _ptr(o_), rows, cols, None))
        torch.cuda.synchronize()
    run(pz(x, 0), win)
    check_windows(f"transpose {rows}x{cols}", [("out", big, win)])
    plain = nans(cols, rows, torch.bfloat16)
    run(x, plain)
    check_equal(f"transpose {rows}x{cols}", [("out", win, plain)])
    same_bits(f"transpose {rows}x{cols}", plain, x.t().contiguous())


@pytest.mark.parametrize("B,H,W,Cc", R.SUMPOOL_CASES)
def test_sumpool2x2(B, H, W, Cc):
    name = f"sumpool {B}x{H}x{W}x{Cc}"
    x = torch.randn(B * 2 * H * 2 * W, Cc, generator=R.gen(61), device="cpu").to(DEV)
    big, win = flat_window((B * H * W, Cc), torch.float32)

    def run(x_, o_):
        chk(_lib().rt_op_sumpool2x2(_ptr(x_), _ptr(o_), B, H, W, Cc, None))
        torch.cuda.synchronize()
    run(pz(x, 0), win)
    check_windows(name, [("out", big, win)])
    plain = nans(B * H * W, Cc)
    run(x, plain)
    check_equal(name, [("out", win, plain)])
    ref, terms = R.sumpool_ref(x.reshape(B, 2 * H, 2 * W, Cc))
    bounded(name, plain.reshape(B, H, W, Cc), ref, 2.0 ** -22 * terms)          # three fp32 additions


# ----------------------------------------------------------------------------------------------- post_quant_conv forward and backward + update
@pytest.mark.parametrize("with_lo", [True, False], ids=["pair", "hi"])
@pytest.mark.parametrize("with_eps", [True, False], ids=["eps", "noeps"])
@pytest.mark.parametrize("HW", R.PQ_HW)
def test_pq_conv_forward(HW, with_eps, with_lo):
    name = f"pq_conv_fwd HW={HW} eps={with_eps} lo={with_lo}"
    lat, eps, W, b, c_lat, c_eps = R.pq_inputs(HW)
    lat, eps, W, b = dev(lat), dev(eps) if with_eps else None, dev(W), dev(b)
    wins = {k: flat_window((HW, 8), torch.bfloat16) for k in (("out", "lo") if with_lo else ("out",))}
    w = {k: vw[1] for k, vw in wins.items()}

    def run(lat_, eps_, W_, b_, o_, l_):
        chk(_lib().rt_op_pq_conv_fwd(_ptr(lat_), _ptr(eps_), F(c_lat), F(c_eps), _ptr(W_), _ptr(b_), _ptr(o_), _ptr(l_), HW, None))
        torch.cuda.synchronize()
    run(pz(lat, 0), pz(eps, 0), pz(W, 0), pz(b), w["out"], w.get("lo"))
    check_windows(name, [(k, bg, vw) for k, (bg, vw) in wins.items()])
    p = {k: nans(HW, 8, torch.bfloat16) for k in w}
    run(lat, eps, W, b, p["out"], p.get("lo"))
    check_equal(name, [(k, w[k], p[k]) for k in w])
    for k in p:                                                     # channels 4..7: exactly +0
        assert not bool(bits(p[k][:, 4:]).any()), f"{name}: {k} channels 4..7 are not zero"
    # the fp32 arithmetic in front of the rounding: c_lat, c_eps as the kernel receives them (fp32)
    ref, terms = R.pq_fwd_ref(lat, eps, float(torch.tensor(c_lat, dtype=torch.float32)), float(torch.tensor(c_eps, dtype=torch.float32)), W, b)
    bounded(name, R.pair64(p["out"], p.get("lo"))[:, :4], ref, (R.PAIR_REL if with_lo else R.HI_REL) * ref.abs() + 2.0 ** -21 * terms)
    if with_lo:
        bounded(name + " hi", p["out"][:, :4], ref, R.HI_REL * ref.abs() + 2.0 ** -21 * terms)


@pytest.mark.parametrize("with_grad", [True, False], ids=["grad_out", "nograd"])
@pytest.mark.parametrize("HW", R.PQ_HW)
def test_pq_conv_backward_update(HW, with_grad):
    name = f"pq_conv_bwd HW={HW} grad_out={with_grad}"
    lat, _, W, _, c_lat, _ = R.pq_inputs(HW)
    g = R.gen(71 + HW)
    dz, mask = dev(torch.randn(HW, 4, generator=g)), dev(torch.rand(4, HW, generator=g))
    lat, W = dev(lat), dev(W)
    gscale, weight = float(torch.tensor(c_lat, dtype=torch.float32)), float(torch.tensor(0.7, dtype=torch.float32))

    def run(dz_, W_, m_, lat_, g_):
        chk(_lib().rt_op_pq_conv_bwd_update(_ptr(dz_), dz_.stride(0), _ptr(W_), F(gscale), F(weight), _ptr(m_), _ptr(lat_), _ptr(g_), HW, None))
        torch.cuda.synchronize()
    (bl, wl), (bg, wg) = flat_window((4, HW), torch.float32), flat_window((4, HW), torch.float32)
    wl.copy_(lat)                                                   # updated in place
    run(pz(dz), pz(W, 0), pz(mask, 0), wl, wg if with_grad else None)
    check_windows(name, [("lat", bl, wl)] + ([("grad_out", bg, wg)] if with_grad else []))
    pl, pg = lat.clone(), nans(4, HW)
    run(dz, W, mask, pl, pg if with_grad else None)
    check_equal(name, [("lat", wl, pl)] + ([("grad_out", wg, pg)] if with_grad else []))
    gr, new, tg, tn = R.pq_bwd_ref(dz, W, gscale, weight, mask, lat)
    bounded(name + " lat", pl, new, 2.0 ** -21 * tn)
    if with_grad:
        bounded(name + " grad_out", pg, gr, 2.0 ** -21 * tg)


# ----------------------------------------------------------------------------------------------- colour loss and gradient
@pytest.mark.parametrize("with_lo", [True, False], ids=["pair", "hi"])
@pytest.mark.parametrize("n", R.COLOR_N)
def test_color_loss_grad(n, with_lo):
    name = f"color n={n} lo={with_lo}"
    HWi = R.COLOR_HWI
    img, masks, target = (dev(t) for t in R.color_inputs(n))
    img4 = torch.cat([img, torch.full((HWi, 1), 1e3, device=DEV)], dim=1).contiguous()      # plain run: channel 3 is finite junk nobody may use
    wins = {k: flat_window((HWi, 8), torch.bfloat16) for k in (("dimg", "lo") if with_lo else ("dimg",))}
    wins["loss"] = guarded((1, 1), torch.float32, device=DEV)
    w = {k: vw[1] for k, vw in wins.items()}

    def run(img_, m_, t_, d_, l_, loss_):
        assert img_.stride(0) == R.COLOR_LDI
        chk(_lib().rt_op_color_loss_grad(_ptr(img_), img_.stride(0), _ptr(m_), _ptr(t_), n, HWi, _ptr(d_), _ptr(l_), _ptr(loss_), None))
        torch.cuda.synchronize()
    run(poisoned(img, R.COLOR_LDI), pz(masks, 0), pz(target, 0), w["dimg"], w.get("lo"), w["loss"])      # contract run: channel 3 is NaN
    check_windows(name, [(k, b, vw) for k, (b, vw) in wins.items()])
    p = {k: nans(*vw.shape, vw.dtype) for k, vw in w.items()}
    run(img4[:, :3], masks, target, p["dimg"], p.get("lo"), p["loss"])
    check_equal(name, [(k, w[k], p[k]) for k in w])
    loss, grad = R.color_ref(img, masks, target)
    judge("color_loss", name, abs(p["loss"].item() - loss.item()) / abs(loss.item()))
    got = R.pair64(p["dimg"], p.get("lo"))
    judge("color_grad", name, R.needed_R(got[:, :3], grad, rel=R.PAIR_REL if with_lo else R.HI_REL))
    # the clamp passes the gradient on the closed interval only; outside (and where no mask reaches) it is exactly zero
    assert torch.equal(got[:, :3] == 0, grad == 0), f"{name}: the zero pattern of the gradient differs from the reference's"
    v = img.double() * 0.5 + 0.5
    edge = (v == 0) | (v == 1)
    assert bool(edge.any()) and bool(((grad != 0) & edge).any()) and bool(((v < 0) | (v > 1)).any())
    for k in ("dimg", "lo") if with_lo else ("dimg",):
        assert not bool(bits(p[k][:, 3:]).any()), f"{name}: {k} channels 3..7 are not zero"
