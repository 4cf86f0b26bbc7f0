"""-m gpu: operator entry points no other op test reaches, each against a plain reference with a per-element criterion:
  * mmhip_op_cast_group (cast_dual_kernel: every weight, every optimizer step) -- exact equality with src.to(dtype) and its transpose, groups that
    straddle CAST_MAX_GROUP (= 4, csrc/mmhip_kernels.h), full and partial 64 x 64 tiles, guard bands, host-side rejects;
  * act == 3 of mmhip_op_gemm_nt (quick-GELU, mm_qgelu: the CLIP tower's MLP) in gemm.hip, gemm8.hip and x3.hip -- against x / (1 + exp(-1.702 x))
    in double with the bound derived in op_bounds.qgelu_bound;
  * mmhip_op_layernorm_fwd with MMHIP_PAIR (the y_pair store of ln_fwd_kernel) -- op_bounds.ln_bounds.
Margins are printed (pytest -s) and tabulated in profiles/op_test_margins.md."""
import ctypes as C

import pytest
import torch

import op_bounds as OB

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gpu_util import DT, dev, ptr, stream, call, assert_close_elementwise, guarded, guards_intact
    from smtc_amd import _lib

CAST_MAX_GROUP = 4          # csrc/mmhip_kernels.h
CAST_SHAPES = [(768, 768), (3072, 768), (4, 4), (68, 132), (64, 4), (4, 2048), (2304, 768), (132, 68), (4, 64)]


@pytest.mark.parametrize("dt", ["bf16", "f16", "x3"])
@pytest.mark.parametrize("count", [1, CAST_MAX_GROUP, CAST_MAX_GROUP + 1, 8, 9])
@pytest.mark.parametrize("with_t", [False, True])
def test_cast_group_is_exact(dt, count, with_t):
    code, tdt = DT[dt]
    g = torch.Generator(device="cpu").manual_seed(count)
    arr = (_lib.CastMat * count)()
    held = []
    for i in range(count):
        rows, cols = CAST_SHAPES[(i + count) % len(CAST_SHAPES)]
        src = torch.randn(rows, cols, generator=g).to(dev())
        d = guarded((rows, cols), tdt, float("nan"))
        t = guarded((cols, rows), tdt, float("nan")) if with_t else None
        arr[i] = _lib.CastMat(src.data_ptr(), d[1].data_ptr(), t[1].data_ptr() if with_t else None, rows, cols)
        held.append((src, d, t))
    call("mmhip_op_cast_group", code, C.cast(arr, C.c_void_p), count, stream())
    torch.cuda.synchronize()
    for src, d, t in held:
        want = src.to(tdt)
        assert torch.equal(d[1], want) and guards_intact(d[0], d[2], want.numel()), tuple(src.shape)
        if with_t:
            assert torch.equal(t[1], want.t().contiguous()) and guards_intact(t[0], t[2], want.numel()), tuple(src.shape)


@pytest.mark.parametrize("rows,cols,null_dst", [(3, 64, False), (64, 3, False), (0, 64, False), (6, 64, False), (64, 70, False), (64, 64, True)])
def test_cast_group_rejects_on_the_host(rows, cols, null_dst):
    """rows / cols below 4 or not multiples of 4, a NULL dst: MMHIP_E_INVALID or a hip error before the launch, destinations untouched"""
    src = torch.randn(max(rows, 4), max(cols, 4), device=dev())
    d = torch.full((128, 128), 3.0, dtype=torch.bfloat16, device=dev())
    t = torch.full((128, 128), 3.0, dtype=torch.bfloat16, device=dev())
    arr = (_lib.CastMat * 1)(_lib.CastMat(src.data_ptr(), None if null_dst else d.data_ptr(), t.data_ptr(), rows, cols))
    rc = _lib.lib().mmhip_op_cast_group(0, C.cast(arr, C.c_void_p), 1, stream())
    torch.cuda.synchronize()
    assert rc == -1 or rc > 0, rc
    assert (d == 3).all() and (t == 3).all()


@pytest.mark.parametrize("dt,slow", [("bf16", 0), ("bf16", 16), ("bf16", 224), ("f16", 256), ("x3", 0)])
def test_quick_gelu_epilogue(dt, slow):
    """act = 3 alone, as test_gelu_epilogue_is_the_erf_gelu does for act = 1: B = I makes the accumulator the (16-bit exact) input, the fp32 output is
    mm_qgelu(x) = x * rcp(1 + __expf(-1.702 x)).  Bound (op_bounds.qgelu_bound): |ref| U_32 (3 + (1 - sigma)(1 + |1.702 x|)) * 2 -- the roundings of
    1 + e, v_rcp and the last product, and those of -1.702 x and __expf scaled by d sigma / d e.  +-30 are inside the same bound: 30 and -30 / (1 + e^51.06)
    = -2e-21 (fp32 holds e^51; a flush to -0 would be outside the relative bound and is not what the kernel does), never NaN."""
    code, tdt = DT[dt]
    M, N = 512, 128
    g = torch.Generator(device="cpu").manual_seed(5)
    x = ((torch.rand(M, N, generator=g) * 18 - 9).to(torch.bfloat16 if dt == "x3" else tdt)).to(tdt)
    x[0, :8] = torch.tensor([0.0, -0.0, 1e-4, -1e-4, 5.5, -5.5, 30.0, -30.0]).to(torch.bfloat16 if dt == "x3" else tdt).to(tdt)      # x3: exact as hi alone
    A, B = x.to(dev()), torch.eye(N, dtype=tdt, device=dev())
    C_ = torch.full((M, N), float("nan"), dtype=torch.float32, device=dev())
    args = lambda: (code, ptr(A), N, ptr(B), N, ptr(C_), N, M, N, N, None, 3, None, 0, None, 0, 0.0, 0, 0, None, 0, 0 if dt == "x3" else 1, slow, stream())
    call("mmhip_op_gemm_nt", *args())
    torch.cuda.synchronize()
    m = assert_close_elementwise(C_, OB.qgelu_reference(x), OB.qgelu_bound(x), f"quick-GELU {dt} slow={slow}")
    print(f"MARGIN qgelu {dt} slow={slow} {m:.4f}")
    c = C_.cpu()
    assert abs(c[0, 6].item() - 30.0) <= 30.0 * 6 * OB.U_32 and -1e-20 < c[0, 7].item() <= 0.0 and not torch.isnan(c[0]).any()
    A[1, 3] = float("nan")
    call("mmhip_op_gemm_nt", *args())
    torch.cuda.synchronize()
    assert torch.isnan(C_[1, 3]).item() and torch.isfinite(C_[0]).all().item()


@pytest.mark.parametrize("rows,width", [(37, 768), (130, 1024), (8192, 768), (5, 4)])
def test_layernorm_forward_plane_pair(rows, width):
    """MMHIP_PAIR: fp32 rows in, y as rows of [hi (width) | lo (width)] bf16.  hi + lo, mean and rstd per element (op_bounds.ln_bounds: fp32 LayerNorm
    + 2^-16 for the pair); the hi plane alone must be the value rounded to bf16.  Row scales alternate 0.05 / 2 so that eps matters on half the rows."""
    g = torch.Generator(device="cpu").manual_seed(rows)
    x = (torch.randn(rows, width, generator=g) * torch.tensor([0.05, 2.0]).repeat(rows // 2 + 1)[:rows, None] + 0.3).float()
    gamma, beta = 1 + 0.1 * torch.randn(width, generator=g), 0.1 * torch.randn(width, generator=g)
    ybuf, y, ysnap = guarded((rows, 2 * width), torch.bfloat16, float("nan"))
    mean, rstd = torch.full((rows,), float("nan"), device=dev()), torch.full((rows,), float("nan"), device=dev())
    xd, gd, bd = x.to(dev()), gamma.to(dev()), beta.to(dev())
    call("mmhip_op_layernorm_fwd", 3, ptr(xd), ptr(y), ptr(gd), ptr(bd), ptr(mean), ptr(rstd), rows, width, 1e-5, stream())
    torch.cuda.synchronize()
    assert guards_intact(ybuf, ysnap, y.numel())
    ref, rmean, rrstd = OB.ln_reference(x, gamma, beta, 1e-5)
    yb, mb, rb = OB.ln_bounds(x, gamma, beta, 1e-5, OB.U_PAIR)
    yc = y.cpu()
    hi, lo = yc[:, :width], yc[:, width:]
    assert OB.pair_hi_is_nearest(hi, lo).all()
    m = (assert_close_elementwise(hi.double() + lo.double(), ref, yb, "y"), assert_close_elementwise(mean, rmean, mb, "mean"),
         assert_close_elementwise(rstd, rrstd, rb, "rstd"))
    print(f"MARGIN ln_pair rows={rows} width={width} y={m[0]:.4f} mean={m[1]:.4f} rstd={m[2]:.4f}")


# ---------------------------------------------------------------------------------------------------------------- composite blocks
# Every tensor a block saves or returns is compared per element with the fp64 operator applied to what the BLOCK ITSELF stored as that stage's
# input (x -> qkv -> att / lse -> pre -> mean / rstd / y, and back): each stage then carries exactly one operator's derived bound
# (op_bounds.gemm_nt_reference, attn_fwd_bounds / attn_bwd_bounds, ln_bounds, ln_bwd_reference), and the chain of stages IS the header's formula and
# its gradient.  Dropout masks are replayed from keep_mask: stream 7 attention probabilities, 8 projection output, 9 FFN output.
BLK_DT = ["bf16", "f16", "x3"]
SEEDB = 0x5EED5


def _t(x64, dt):
    return x64.to(DT[dt][1]).to(dev()).contiguous()


def _rt(shape, g, dt, scale=1.0):
    """random values the dtype holds exactly (fp64 on the CPU)"""
    return OB.rnd((torch.randn(*shape, generator=g) * scale).double(), dt)


def _chk(got, ref, bound, what, margins):
    margins.append(assert_close_elementwise(got, ref, bound, what))


def _keep(shape, sid, p):
    from gpu_util import keep_mask
    return (None, 1.0) if p == 0 else keep_mask(shape, sid, SEEDB, p)


def _ln_fwd_check(pre, gamma, beta, eps, dt, y, mean, rstd, ms):
    p64 = pre.double().cpu()
    ref, rmean, rrstd = OB.ln_reference(p64, gamma, beta, eps)
    yb, mb, rb = OB.ln_bounds(p64, gamma, beta, eps, OB.FMT[dt].u_out)
    _chk(y, ref, yb, "y", ms), _chk(mean, rmean, mb, "mean", ms), _chk(rstd, rrstd, rb, "rstd", ms)


def _ln_bwd_check(dy64, pre, gamma, mean, rstd, keep, scale, dt, dpre, dd, dd_snap, dg, db, dg0, db0, ms):
    u = OB.FMT[dt].u_out
    dx, dx_e, _, dgam, dgam_b, dbet, dbet_b = OB.ln_bwd_reference(dy64, pre.double().cpu(), gamma, mean.cpu(), rstd.cpu())
    _chk(dpre, dx, OB.SLACK * (dx_e + u * dx.abs()), "dpre", ms)
    if keep is None:
        assert torch.equal(dd.view(torch.int32 if dd.element_size() == 4 else torch.int16), dd_snap.view(torch.int32 if dd.element_size() == 4 else torch.int16)), "dd written although p_hid == 0"
    else:
        ref = dpre.double().cpu() * keep.double() * scale          # dd = the stored dpre, dropped and scaled
        dxk = dx * keep.double() * scale                            # ... or the unrounded one: either reading is inside  (2 U_32 + 2 u) |dd|
        _chk(dd, dxk, OB.SLACK * ((dx_e + u * dx.abs()) * keep.double() * scale + (2 * OB.U_32 + u) * dxk.abs()), "dd", ms)
        assert ((dd.double().cpu() == 0) | keep).all() and ref.shape == dxk.shape
    _chk(dg, dg0.double() + dgam, dgam_b + OB.SLACK * OB.U_32 * (dg0.double().abs() + dgam.abs()), "dgamma (added)", ms)
    _chk(db, db0.double() + dbet, dbet_b + OB.SLACK * OB.U_32 * (db0.double().abs() + dbet.abs()), "dbeta (added)", ms)


def _tn_closure(dt, probs, ms):
    """the weight-gradient operands the block leaves behind, through mmhip_op_gemm_tn_group: C = A^T B and the bias column sums against fp64 of the
    same operands:  split_err + M U_32 |A|^T |B| + U_32 |C|, times SLACK"""
    code = DT[dt][0]
    arr = (_lib.TNProblem * len(probs))()
    outs = []
    for i, (A, lda, Nn, B, ldb, Nc, M) in enumerate(probs):
        Cw, cs = torch.zeros(Nn, Nc, device=dev()), torch.zeros(Nn, device=dev())
        arr[i] = _lib.TNProblem(A.data_ptr(), B.data_ptr(), Cw.data_ptr(), M, Nn, Nc, lda, ldb, Nc, cs.data_ptr())
        outs.append((Cw, cs))
    call("mmhip_op_gemm_tn_group", code, C.cast(arr, C.c_void_p), len(probs), 0, stream())
    torch.cuda.synchronize()
    fmt = OB.FMT[dt]
    for (A, lda, Nn, B, ldb, Nc, M), (Cw, cs) in zip(probs, outs):
        a, b = A.double().cpu()[:, :Nn], B.double().cpu()[:, :Nc]
        ref = a.t() @ b
        bound = OB.SLACK * (OB.split_err(fmt, a.t(), b.t()) + M * OB.U_32 * (a.abs().t() @ b.abs()) + OB.U_32 * ref.abs())
        _chk(Cw, ref, bound, "weight gradient", ms)
        _chk(cs, a.sum(0), OB.SLACK * (M * OB.U_32 * a.abs().sum(0) + OB.U_32 * a.sum(0).abs()) + 1e-300, "bias gradient", ms)


@pytest.mark.parametrize("dt", BLK_DT)
@pytest.mark.parametrize("heads", [1, 12])
@pytest.mark.parametrize("posts,S", [(3, 20), (2, 128), (5, 36)])
@pytest.mark.parametrize("p_att,p_hid", [(0.0, 0.0), (0.1, 0.0), (0.0, 0.1), (0.1, 0.1)])
def test_self_attention_block(dt, heads, posts, S, p_att, p_hid):
    code, tdt = DT[dt]
    H, M, eps = heads * 64, posts * S, 1e-12
    g = torch.Generator(device="cpu").manual_seed(posts * 1000 + S + heads)
    x, wqkv, wo = _rt((M, H), g, dt), _rt((3 * H, H), g, dt, H ** -0.5), _rt((H, H), g, dt, H ** -0.5)
    bqkv, bo = 0.1 * torch.randn(3 * H, generator=g), 0.1 * torch.randn(H, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    lens = torch.randint(1, S + 1, (posts,), generator=g)
    lens[0] = S
    maskbias = torch.where(torch.arange(S)[None, :] < lens[:, None], 0.0, float("-inf")).float().contiguous()
    dy = _rt((M, H), g, dt)
    d = lambda t: t.to(dev()).contiguous()
    X, Wqkv, Wo, WqkvT, WoT, DY = _t(x, dt), _t(wqkv, dt), _t(wo, dt), _t(wqkv.t(), dt), _t(wo.t(), dt), _t(dy, dt)
    Bq, Bo, G, Be, MB = d(bqkv), d(bo), d(gamma), d(beta), d(maskbias)
    nan = lambda *s, **k: torch.full(s, float("nan"), device=dev(), **k)
    qkv, att, pre, y = nan(M, 3 * H, dtype=tdt), nan(M, H, dtype=tdt), nan(M, H, dtype=tdt), nan(M, H, dtype=tdt)
    lse, mean, rstd = nan(posts, heads, S), nan(M), nan(M)
    call("mmhip_op_self_att_block_fwd", code, ptr(X), ptr(MB), ptr(Wqkv), ptr(Bq), ptr(Wo), ptr(Bo), ptr(G), ptr(Be), eps, posts, S, heads, p_att, p_hid, SEEDB,
         ptr(qkv), ptr(att), ptr(lse), ptr(pre), ptr(mean), ptr(rstd), ptr(y), stream())
    torch.cuda.synchronize()
    ms = []
    ref, b, _, _ = OB.gemm_nt_reference(x, wqkv, dt, bias=bqkv)
    _chk(qkv, ref, b, "qkv", ms)
    k7, s7 = _keep((posts, heads, S, S), 7, p_att)
    k8, s8 = _keep((M, H), 8, p_hid)
    r = OB.attn_reference(qkv.double().cpu(), maskbias, posts, S, heads, k7, s7)
    ctx_b, lse_b = OB.attn_fwd_bounds(r, dt, S)
    _chk(att, OB.to_rows(r.ctx), OB.to_rows(ctx_b), "att", ms), _chk(lse, r.lse, lse_b, "lse", ms)
    ref, b, _, _ = OB.gemm_nt_reference(att.double().cpu(), wo, dt, bias=bo, keep=k8, scale=s8, resid=x)
    _chk(pre, ref, b, "pre", ms)
    _ln_fwd_check(pre, gamma, beta, eps, dt, y, mean, rstd, ms)
    # ---- backward
    dg0, db0 = torch.randn(H, generator=g), torch.randn(H, generator=g)
    dg, db = d(dg0), d(db0)
    dpre, datt, dqkv, dx = nan(M, H, dtype=tdt), nan(M, H, dtype=tdt), nan(M, 3 * H, dtype=tdt), nan(M, H, dtype=tdt)
    dd = torch.full((M, H), 7.0, dtype=tdt, device=dev())
    dd_snap = dd.clone()
    call("mmhip_op_self_att_block_bwd", code, ptr(DY), ptr(MB), ptr(WqkvT), ptr(WoT), ptr(G), posts, S, heads, p_att, p_hid, SEEDB, ptr(qkv), ptr(att), ptr(lse),
         ptr(pre), ptr(mean), ptr(rstd), ptr(dg), ptr(db), ptr(dpre), ptr(dd), ptr(datt), ptr(dqkv), ptr(dx), stream())
    torch.cuda.synchronize()
    _ln_bwd_check(dy, pre, gamma, mean, rstd, k8, s8, dt, dpre, dd, dd_snap, dg, db, dg0, db0, ms)
    dsrc = dd if p_hid > 0 else dpre
    ref, b, _, _ = OB.gemm_nt_reference(dsrc.double().cpu(), wo.t(), dt)
    _chk(datt, ref, b, "datt", ms)
    rb = OB.attn_reference(qkv.double().cpu(), maskbias, posts, S, heads, k7, s7, datt.double().cpu())
    bq, bk, bv = OB.attn_bwd_bounds(rb, dt, S, ctx_err=ctx_b, lse_err=lse_b)
    got = dqkv.double().cpu()
    for i, (name, rr, bb) in enumerate((("dq", rb.dq, bq), ("dk", rb.dk, bk), ("dv", rb.dv, bv))):
        _chk(got[:, i * H:(i + 1) * H], OB.to_rows(rr), OB.to_rows(bb), name, ms)
    ref, b, _, _ = OB.gemm_nt_reference(got, wqkv.t(), dt, resid=dpre.double().cpu())
    _chk(dx, ref, b, "dx", ms)
    _tn_closure(dt, [(dsrc, H, H, att, H, H, M), (dqkv, 3 * H, 3 * H, X, H, H, M)], ms)
    print(f"MARGIN self_att_block {dt} heads={heads} posts={posts} S={S} p_att={p_att} p_hid={p_hid} worst={max(ms):.4f}")


@pytest.mark.parametrize("dt", BLK_DT)
@pytest.mark.parametrize("M,H,I", [(60, 64, 256), (256, 768, 3072), (37, 768, 3072)])
@pytest.mark.parametrize("p_hid", [0.0, 0.1])
def test_ffn_block(dt, M, H, I, p_hid):
    code, tdt = DT[dt]
    eps = 1e-12
    g = torch.Generator(device="cpu").manual_seed(M + I)
    x, w1, w2 = _rt((M, H), g, dt), _rt((I, H), g, dt, H ** -0.5), _rt((H, I), g, dt, I ** -0.5)
    b1, b2 = 0.1 * torch.randn(I, generator=g), 0.1 * torch.randn(H, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(H, generator=g), 0.1 * torch.randn(H, generator=g)
    dy = _rt((M, H), g, dt)
    d = lambda t: t.to(dev()).contiguous()
    X, W1, W2, W1T, W2T, DY = _t(x, dt), _t(w1, dt), _t(w2, dt), _t(w1.t(), dt), _t(w2.t(), dt), _t(dy, dt)
    B1, B2, G, Be = d(b1), d(b2), d(gamma), d(beta)
    nan = lambda *s, **k: torch.full(s, float("nan"), device=dev(), **k)
    h, u, pre, y, mean, rstd = nan(M, I, dtype=tdt), nan(M, I, dtype=tdt), nan(M, H, dtype=tdt), nan(M, H, dtype=tdt), nan(M), nan(M)
    call("mmhip_op_ffn_block_fwd", code, ptr(X), ptr(W1), ptr(B1), ptr(W2), ptr(B2), ptr(G), ptr(Be), eps, M, H, I, p_hid, SEEDB, ptr(h), ptr(u), ptr(pre), ptr(mean),
         ptr(rstd), ptr(y), stream())
    torch.cuda.synchronize()
    ms = []
    ref, b, pref, pb = OB.gemm_nt_reference(x, w1, dt, bias=b1, act=1)
    _chk(h, ref, b, "h", ms), _chk(u, pref, pb, "u", ms)
    k9, s9 = _keep((M, H), 9, p_hid)
    ref, b, _, _ = OB.gemm_nt_reference(h.double().cpu(), w2, dt, bias=b2, keep=k9, scale=s9, resid=x)
    _chk(pre, ref, b, "pre", ms)
    _ln_fwd_check(pre, gamma, beta, eps, dt, y, mean, rstd, ms)
    dg0, db0 = torch.randn(H, generator=g), torch.randn(H, generator=g)
    dg, db = d(dg0), d(db0)
    dpre, du, dx = nan(M, H, dtype=tdt), nan(M, I, dtype=tdt), nan(M, H, dtype=tdt)
    dd = torch.full((M, H), 7.0, dtype=tdt, device=dev())
    dd_snap = dd.clone()
    call("mmhip_op_ffn_block_bwd", code, ptr(DY), ptr(W1T), ptr(W2T), ptr(G), M, H, I, p_hid, SEEDB, ptr(u), ptr(pre), ptr(mean), ptr(rstd), ptr(dg), ptr(db), ptr(dpre),
         ptr(dd), ptr(du), ptr(dx), stream())
    torch.cuda.synchronize()
    _ln_bwd_check(dy, pre, gamma, mean, rstd, k9, s9, dt, dpre, dd, dd_snap, dg, db, dg0, db0, ms)
    dsrc = dd if p_hid > 0 else dpre
    ref, b, _, _ = OB.gemm_nt_reference(dsrc.double().cpu(), w2.t(), dt, mulg=u.double().cpu())
    _chk(du, ref, b, "du", ms)
    ref, b, _, _ = OB.gemm_nt_reference(du.double().cpu(), w1.t(), dt, resid=dpre.double().cpu())
    _chk(dx, ref, b, "dx", ms)
    _tn_closure(dt, [(dsrc, H, H, h, I, I, M), (du, I, I, X, H, H, M)], ms)
    print(f"MARGIN ffn_block {dt} M={M} H={H} I={I} p_hid={p_hid} worst={max(ms):.4f}")


# ---------------------------------------------------------------------------------------------------------------- strided mmhip_op_gemm_nt
def _padded(x64, ld, tdt, fill):
    """[rows, cols] inside a [rows, ld] buffer whose pad columns hold `fill` (NaN for operands: a read past K poisons the result; a sentinel for
    outputs: a write past N shows)"""
    rows, cols = x64.shape
    buf = torch.full((rows, ld), fill, dtype=tdt, device=dev())
    buf[:, :cols] = x64.to(tdt).to(dev())
    return buf


STRIDED = [(96, 48, 64, 1), (256, 256, 128, 16), (200, 128, 64, 224), (2048, 256, 64, 240), (300, 384, 192, 336)]


@pytest.mark.parametrize("dt,M,N,K,slow", [(dt, *s) for dt in ("bf16", "f16") for s in STRIDED] + [("x3", 300, 132, 96, 0), ("x3", 64, 128, 256, 0)])
def test_gemm_nt_strided(dt, M, N, K, slow):
    """lda = ldb = K + 8, ldc = N + 16, ldaux = N + 8, ldres = N + 24, ldmul = N + 8, the five epilogues of test_gemm_nt_epilogues per element
    (op_bounds.gemm_nt_reference).  Pad columns of A / B hold NaN, those of C / aux a sentinel that must survive.  A launcher that rejects a stride on
    the host must say so (MMHIP_E_INVALID / a hip error) and leave C alone.  Dropped-element identity: C - residual is exactly 0 where the mask drops;
    kept elements that also read 0 (below half an output ulp of the residual) are at most 1 %."""
    code, tdt = DT[dt]
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A, B = _rt((M, K), g, dt, 0.5), _rt((N, K), g, dt, 0.05)
    bias = torch.randn(N, generator=g)
    resid, mulg = _rt((M, N), g, dt), _rt((M, N), g, dt)
    Ad, Bd = _padded(A, K + 8, tdt, float("nan")), _padded(B, K + 8, tdt, float("nan"))
    Rd, Ud, biasd = _padded(resid, N + 24, tdt, float("nan")), _padded(mulg, N + 8, tdt, float("nan")), bias.to(dev())
    seed, sid, ms = 0x123456789ABCDEF, 21, []
    from gpu_util import keep_mask
    for variant in ("plain", "bias_gelu_aux", "bias_drop_resid", "mulgrad_resid", "bias_tanh_f32"):
        f32 = variant == "bias_tanh_f32"
        ctd = torch.float32 if f32 else tdt
        Cd = torch.full((M, N + 16), 5.0, dtype=ctd, device=dev())
        auxd = torch.full((M, N + 8), 5.0, dtype=tdt, device=dev())
        kw = dict(bias=None, act=0, aux=None, mulg=None, p=0.0, resid=None)
        if variant == "bias_gelu_aux":
            kw.update(bias=biasd, act=1, aux=auxd)
        if variant == "bias_drop_resid":
            kw.update(bias=biasd, p=0.1, resid=Rd)
        if variant == "mulgrad_resid":
            kw.update(mulg=Ud, resid=Rd)
        if f32:
            kw.update(bias=biasd, act=2)
        rc = _lib.lib().mmhip_op_gemm_nt(code, ptr(Ad), K + 8, ptr(Bd), K + 8, ptr(Cd), N + 16, M, N, K, ptr(kw["bias"]), kw["act"], ptr(kw["aux"]), N + 8,
                                         ptr(kw["mulg"]), N + 8, kw["p"], seed, sid, ptr(kw["resid"]), N + 24, 1 if f32 else 0, slow, stream())
        torch.cuda.synchronize()
        if rc != 0:
            assert rc == -1 or rc > 0
            assert (Cd == 5).all() and (auxd == 5).all(), "rejected, yet written"
            print(f"MARGIN gemm_nt_strided {dt} {M}x{N}x{K} slow={slow} {variant} rejected rc={rc}")
            continue
        keep, scale = (None, 1.0) if kw["p"] == 0 else keep_mask((M, N), sid, seed, kw["p"])
        ref, b, pre, pb = OB.gemm_nt_reference(A, B, dt, bias=None if kw["bias"] is None else bias, act=kw["act"], mulg=None if kw["mulg"] is None else mulg,
                                               keep=keep, scale=scale, resid=None if kw["resid"] is None else resid, out="f32" if f32 else "t")
        assert (Cd[:, N:] == 5).all() and (auxd[:, N:] == 5).all(), "pad columns written"
        _chk(Cd[:, :N], ref, b, f"C {variant}", ms)
        if kw["aux"] is not None:
            _chk(auxd[:, :N], pre, pb, "aux", ms)
        if keep is not None:
            z = (Cd[:, :N].double().cpu() - resid) == 0
            assert z[~keep].all(), "a dropped element is not exactly the residual"
            assert (z & keep).double().mean().item() <= 0.01
    print(f"MARGIN gemm_nt_strided {dt} {M}x{N}x{K} slow={slow} worst={max(ms) if ms else 0:.4f}")


@pytest.mark.parametrize("dt", BLK_DT)
def test_gemm_nt_into_a_column_block_of_a_wider_buffer(dt):
    """the cross-attention block's pattern: C = columns [H, 3H) of a [M, 3H] buffer (N = 2H, ldc = 3H), B = rows [H, 3H) of the fused weight; columns
    [0, H) of the buffer must stay as they were"""
    code, tdt = DT[dt]
    M, H = 150, 128
    g = torch.Generator(device="cpu").manual_seed(4)
    x, w, bias = _rt((M, H), g, dt), _rt((3 * H, H), g, dt, H ** -0.5), torch.randn(3 * H, generator=g)
    X, W, Bd = _t(x, dt), _t(w, dt), bias.to(dev())
    buf = torch.full((M, 3 * H), 5.0, dtype=tdt, device=dev())
    Z = buf.element_size()
    rc = _lib.lib().mmhip_op_gemm_nt(code, ptr(X), H, C.c_void_p(W.data_ptr() + H * H * Z), H, C.c_void_p(buf.data_ptr() + H * Z), 3 * H, M, 2 * H, H,
                                     C.c_void_p(Bd.data_ptr() + 4 * H), 0, None, 0, None, 0, 0.0, 0, 0, None, 0, 0, 0, stream())
    torch.cuda.synchronize()
    assert rc == 0 and (buf[:, :H] == 5).all()
    ref, b, _, _ = OB.gemm_nt_reference(x, w[H:], dt, bias=bias[H:])
    m = assert_close_elementwise(buf[:, H:], ref, b, "C at a column offset")
    print(f"MARGIN gemm_nt_offset {dt} worst={m:.4f}")
