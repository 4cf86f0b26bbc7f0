"""No GPU: the per-element bounds of tests/op_bounds.py are neither too narrow nor uselessly wide.  Per operator family and dtype, for a fixed seed:
  * a CPU emulation of the kernel's roundings (the fp64 reference with the operand / P / dS / output casts inserted) stays INSIDE the bound;
  * a deliberately off-by-one reference (one key dropped, the score scale off by 2^-6, the next dropout stream, eps omitted, 1.7 for 1.702, one 4 x 4
    block left untransposed) lands OUTSIDE it on at least one element.
The second point is what makes a passing -m gpu run (tests/test_gpu_ops_attention.py, tests/test_gpu_ops_blocks.py) mean something."""
import pytest
import torch

import op_bounds as OB
from gpu_util import assert_close_elementwise, violates_elementwise, keep_mask

ATT_DT = ["bf16", "f16", "x3", "pair", "alu"]
POSTS, S, HEADS = 3, 33, 2


def _case(dt, p=0.0, sid=16, with_dctx=False, **kw):
    qkv, dctx, maskbias = OB.attn_inputs(dt, POSTS, S, HEADS, True, seed=3, with_dctx=with_dctx)
    keep, scale = (None, 1.0) if p == 0 else keep_mask((POSTS, HEADS, S, S), sid, 77, p)
    return OB.attn_reference(qkv, maskbias, POSTS, S, HEADS, keep, scale, dctx, **kw)


@pytest.mark.parametrize("dt", ATT_DT)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_forward_bound(dt, p):
    r = _case(dt, p)
    ctx_b, lse_b = OB.attn_fwd_bounds(r, dt, S)
    ctx, lse, *_ = OB.attn_emulate(r, dt)
    assert assert_close_elementwise(ctx, r.ctx, ctx_b, "emulated ctx") <= 1 and assert_close_elementwise(lse, r.lse, lse_b, "emulated lse") <= 1
    wrong = [_case(dt, p, drop_last_key_of=(0, 1)), _case(dt, p, score_scale=0.125 * (1 + 2.0 ** -6))]
    if p:
        wrong.append(_case(dt, p, sid=17))
    for w in wrong:
        assert violates_elementwise(w.ctx, r.ctx, ctx_b) > 0
    assert violates_elementwise(wrong[0].lse, r.lse, lse_b) > 0 and violates_elementwise(wrong[1].lse, r.lse, lse_b) > 0


@pytest.mark.parametrize("dt", ATT_DT)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_attention_backward_bound(dt, p):
    r = _case(dt, p, with_dctx=True)
    bounds = OB.attn_bwd_bounds(r, dt, S)
    _, _, dq, dk, dv = OB.attn_emulate(r, dt)
    for name, got, ref, b in zip(("dq", "dk", "dv"), (dq, dk, dv), (r.dq, r.dk, r.dv), bounds):
        assert assert_close_elementwise(got, ref, b, "emulated " + name) <= 1
    dead = ~r.live[:, :, 0, :]                                  # masked keys: the bound is 0, exact zeros are required
    assert dead.any() and (bounds[1][dead] == 0).all() and (bounds[2][dead] == 0).all()
    wrong = [_case(dt, p, with_dctx=True, drop_last_key_of=(0, 1)), _case(dt, p, with_dctx=True, score_scale=0.125 * (1 + 2.0 ** -6))]
    if p:
        wrong.append(_case(dt, p, sid=17, with_dctx=True))
    for w in wrong:
        for got, ref, b in zip((w.dq, w.dk, w.dv), (r.dq, r.dk, r.dv), bounds):
            assert violates_elementwise(got, ref, b) > 0


def test_quick_gelu_bound():
    g = torch.Generator(device="cpu").manual_seed(5)
    x = (torch.rand(512, 128, generator=g) * 18 - 9).to(torch.bfloat16).double()
    ref, b = OB.qgelu_reference(x), OB.qgelu_bound(x)
    xf = x.float()
    emu = xf * (1.0 / (1.0 + torch.exp(-1.702 * xf)))            # fp32 all the way
    assert assert_close_elementwise(emu, ref, b, "fp32 quick-GELU") <= 1
    assert violates_elementwise(OB.qgelu_reference(x, 1.7), ref, b) > 0


def test_layernorm_pair_bound():
    g = torch.Generator(device="cpu").manual_seed(9)
    x = (torch.randn(37, 768, generator=g) * torch.tensor([0.05, 2.0]).repeat(19)[:37, None] + 0.3).float()
    gamma, beta = 1 + 0.1 * torch.randn(768, generator=g), 0.1 * torch.randn(768, generator=g)
    y, mean, rstd = OB.ln_reference(x, gamma, beta, 1e-5)
    yb, mb, rb = OB.ln_bounds(x, gamma, beta, 1e-5, OB.U_PAIR)
    emu = torch.nn.functional.layer_norm(x, (768,), gamma, beta, 1e-5)
    hi, lo = OB.split_pair(emu)
    assert assert_close_elementwise(hi.double() + lo.double(), y, yb, "fp32 LayerNorm as a plane pair") <= 1
    assert OB.pair_hi_is_nearest(hi, lo).all()
    assert not OB.pair_hi_is_nearest(hi + hi.abs() * 2.0 ** -7, lo).all()          # hi off by one ulp: seen
    y0, _, rstd0 = OB.ln_reference(x, gamma, beta, 0.0)
    assert violates_elementwise(y0, y, yb) > 0 and violates_elementwise(rstd0, rstd, rb) > 0


def test_exact_transposed_copy_sees_one_untransposed_block():
    """mmhip_op_cast_group is held to exact equality; a 4 x 4 sub-block left untransposed differs (random data: with certainty)"""
    g = torch.Generator(device="cpu").manual_seed(2)
    src = torch.randn(68, 132, generator=g)
    good = src.to(torch.bfloat16).t().contiguous()
    bad = good.clone()
    bad[64:68, 4:8] = src.to(torch.bfloat16)[4:8, 64:68]
    assert not torch.equal(bad, good)


def test_assert_close_elementwise_reports_the_worst_element():
    ref, bound = torch.zeros(4, 5, dtype=torch.float64), torch.full((4, 5), 1e-3, dtype=torch.float64)
    got = ref.clone()
    got[2, 3] = 5e-4
    assert abs(assert_close_elementwise(got, ref, bound, "x") - 0.5) < 1e-12
    got[1, 4] = 3e-3
    with pytest.raises(AssertionError, match=r"\(1, 4\).*ratio 3"):
        assert_close_elementwise(got, ref, bound, "x")
    got[1, 4] = float("nan")
    with pytest.raises(AssertionError):
        assert_close_elementwise(got, ref, bound, "x")
    bound[0, 0] = 0.0                              # zero bound: exact match required
    got[1, 4] = 0.0
    assert assert_close_elementwise(got, ref, bound, "x") <= 1
    got[0, 0] = 1e-30
    with pytest.raises(AssertionError):
        assert_close_elementwise(got, ref, bound, "x")


@pytest.mark.parametrize("dt", ["bf16", "f16", "x3"])
def test_gemm_epilogue_bound_and_dropped_element_identity(dt):
    """the bound of op_bounds.gemm_nt_reference (strided GEMM, the blocks' projections): an fp32 product of the same operands, rounded as stored, is
    inside; the next dropout stream and a bias left off one column are outside.  Dropped-element identity at the test's input scales: in the fp64
    reference fewer than 1 % of the KEPT elements lie below one output ulp of the residual (those would read as dropped)."""
    M, N, K = 200, 128, 64
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A, B = OB.rnd((torch.randn(M, K, generator=g) * 0.5).double(), dt), OB.rnd((torch.randn(N, K, generator=g) * 0.05).double(), dt)
    bias, resid = torch.randn(N, generator=g), OB.rnd(torch.randn(M, N, generator=g).double(), dt)
    keep, scale = keep_mask((M, N), 21, 0x123456789ABCDEF, 0.1)
    ref, b, _, _ = OB.gemm_nt_reference(A, B, dt, bias=bias, keep=keep, scale=scale, resid=resid)
    mm = (lambda a, c: OB.operand(a, dt) @ OB.operand(c, dt).t()) if dt == "x3" else (lambda a, c: (a.float() @ c.float().t()).double())
    emu = OB.rnd((((mm(A, B).float() + bias).float() * keep * scale).float() + resid.float()).double(), dt)
    assert assert_close_elementwise(emu, ref, b, "emulated epilogue") <= 1
    keep2, _ = keep_mask((M, N), 22, 0x123456789ABCDEF, 0.1)
    bias2 = bias.clone()
    bias2[5] = 0
    for w in (OB.gemm_nt_reference(A, B, dt, bias=bias, keep=keep2, scale=scale, resid=resid)[0], OB.gemm_nt_reference(A, B, dt, bias=bias2, keep=keep, scale=scale, resid=resid)[0]):
        assert violates_elementwise(w, ref, b) > 0
    u = OB.FMT[dt].u_out
    small = ((ref - resid).abs() < u * resid.abs()) & keep
    assert small.double().mean().item() < 0.01


def test_layernorm_backward_bound():
    g = torch.Generator(device="cpu").manual_seed(13)
    R, W = 37, 768
    x = (torch.randn(R, W, generator=g) * 2 + 0.3).float()
    dy, gamma = torch.randn(R, W, generator=g).float(), 1 + 0.1 * torch.randn(W, generator=g)
    _, mean, rstd = OB.ln_reference(x, gamma, torch.zeros(W), 1e-12)
    mean, rstd = mean.float(), rstd.float()
    dx, dx_e, _, dgam, dgam_b, dbet, dbet_b = OB.ln_bwd_reference(dy, x, gamma, mean, rstd)
    xf = x.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xf, (W,), gamma, None, 1e-12).backward(dy)          # fp32 autograd as the emulation
    assert assert_close_elementwise(xf.grad, dx, OB.SLACK * (dx_e + OB.U_32 * dx.abs()), "fp32 LayerNorm backward") <= 1
    wrong = OB.ln_bwd_reference(dy, x, gamma, mean, rstd * (1 + 2.0 ** -12))
    assert violates_elementwise(wrong[0], dx, OB.SLACK * (dx_e + OB.U_32 * dx.abs())) > 0
    assert violates_elementwise(wrong[3], dgam, dgam_b) > 0


# ---------------------------------------------------------------------------------------------------------------- GEMM NT / TN, column sums, LayerNorm edges
def _nt_emulate(A, B, dt):
    """the accumulator as the kernel forms it: an fp32 product of the operands as the matrix cores read them"""
    if dt == "x3":
        return (OB.operand(A, dt) @ OB.operand(B, dt).t()).float()
    return A.float() @ B.float().t()


@pytest.mark.parametrize("dt", ["bf16", "f16", "x3"])
def test_gemm_nt_bound_sees_a_dropped_k_element(dt):
    """op_bounds.gemm_nt_reference at the GPU tests' operand scales (A ~ 0.5, B ~ 0.05, residual ~ 1): the emulated kernel is inside for the bare fp32
    accumulator (plain_f32), the plain 16-bit store and bias + residual; a reference that loses the last K element, the last 32 of K, or adds the
    neighbouring column's bias is outside somewhere -- for every output type, which is what the scales were chosen for.  The products of one (A, B) are
    computed once (gemm_nt_products) and give the same reference as the one-step call."""
    M, N, K = 200, 128, 128
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A, B = OB.rnd((torch.randn(M, K, generator=g) * 0.5).double(), dt), OB.rnd((torch.randn(N, K, generator=g) * 0.05).double(), dt)
    bias, resid = torch.randn(N, generator=g), OB.rnd(torch.randn(M, N, generator=g).double(), dt)
    pr = OB.gemm_nt_products(A, B, dt)
    acc = _nt_emulate(A, B, dt)
    cases = {"plain_f32": (dict(out="f32"), acc.double()),
             "plain": (dict(), OB.rnd(acc.double(), dt)),
             "bias_resid": (dict(bias=bias, resid=resid), OB.rnd(((acc + bias).float() + resid.float()).double(), dt))}
    for name, (kw, emu) in cases.items():
        ref, b, _, _ = OB.gemm_nt_reference(None, None, dt, products=pr, **kw)
        one_step = OB.gemm_nt_reference(A, B, dt, **kw)
        assert torch.equal(ref, one_step[0]) and torch.equal(b, one_step[1]), name
        assert assert_close_elementwise(emu, ref, b, "emulated " + name) <= 1
        wrong = {"last K element dropped": OB.gemm_nt_reference(A[:, :-1], B[:, :-1], dt, **kw)[0],
                 "last 32 of K dropped": OB.gemm_nt_reference(A[:, :-32], B[:, :-32], dt, **kw)[0]}
        if "bias" in kw:
            wrong["bias of the neighbouring column"] = OB.gemm_nt_reference(None, None, dt, products=pr, **dict(kw, bias=torch.roll(bias, 1)))[0]
        for what, w in wrong.items():
            assert violates_elementwise(w, ref, b) > 0, (name, what)


@pytest.mark.parametrize("dt", ["bf16", "f16", "x3"])
@pytest.mark.parametrize("accumulate", [False, True])
def test_gemm_tn_bound_sees_one_row(dt, accumulate):
    """op_bounds.gemm_tn_reference: fp32 products of the operands as read (+ the accumulate add), stored as fp32, are inside for C and the column sums;
    one row more or one row fewer in the reduction is outside, for C and for the column sums"""
    M, Nn, Nc = 64, 40, 72
    g = torch.Generator(device="cpu").manual_seed(M + Nn)
    A, B = OB.rnd((torch.randn(M + 1, Nn, generator=g) * 0.1).double(), dt), OB.rnd((torch.randn(M + 1, Nc, generator=g) * 0.5).double(), dt)
    C0 = torch.randn(Nn, Nc, generator=g) if accumulate else None
    cs0 = torch.randn(Nn, generator=g) if accumulate else None
    ref, b, cs, csb = OB.gemm_tn_reference(A[:M], B[:M], dt, C0, cs0)
    a, bb = (OB.operand(A[:M], dt), OB.operand(B[:M], dt)) if dt == "x3" else (A[:M], B[:M])
    emu, emu_cs = (a.t() @ bb).float(), a.sum(0).float()
    if accumulate:
        emu, emu_cs = (emu + C0).float(), (emu_cs + cs0).float()
    assert assert_close_elementwise(emu, ref, b, "emulated C") <= 1 and assert_close_elementwise(emu_cs, cs, csb, "emulated column sums") <= 1
    for rows in (M + 1, M - 1):
        w = OB.gemm_tn_reference(A[:rows], B[:rows], dt, C0, cs0)
        assert violates_elementwise(w[0], ref, b) > 0 and violates_elementwise(w[2], cs, csb) > 0, rows


@pytest.mark.parametrize("dt", ["bf16", "f16", "x3"])
def test_colsum_bound_sees_one_row(dt):
    R, Wd = 1000, 36
    g = torch.Generator(device="cpu").manual_seed(R)
    x = OB.rnd(torch.randn(R + 1, Wd, generator=g).double(), dt)
    ref, b = OB.colsum_reference(x[:R])
    assert assert_close_elementwise(x[:R].float().sum(0), ref, b, "fp32 column sums") <= 1
    chunks = torch.stack([x[:R][i:i + 64].float().sum(0) for i in range(0, R, 64)]).sum(0)          # per 64-row chunk, then across chunks
    assert assert_close_elementwise(chunks, ref, b, "chunked fp32 column sums") <= 1
    for rows in (R + 1, R - 1):
        assert violates_elementwise(OB.colsum_reference(x[:rows])[0], ref, b) > 0


def _ln_emulate(x, gamma, beta, eps):
    """ln_fwd_kernel's order in fp32: mean, then the sum of squared differences from it, rsqrt, (x - mean) rstd gamma + beta"""
    x = x.float()
    W = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / W
    d = x - mean
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / W + eps)
    return d * rstd * gamma.float() + beta.float(), mean.squeeze(-1), rstd.squeeze(-1)


@pytest.mark.parametrize("dt", ["bf16", "f16", "x3"])
@pytest.mark.parametrize("width", [768, 4])
def test_layernorm_bound_holds_on_large_mean_and_constant_rows(dt, width):
    """rows with mean 1e3 and unit spread, and a constant row (variance 0: rstd = 1 / sqrt(eps), y = beta), are inside ln_bounds for the fp32 emulation
    rounded as stored; eps left out is outside on the constant row (rstd) and an off-by-one width in the mean is outside on the large-mean rows"""
    g = torch.Generator(device="cpu").manual_seed(width)
    x = OB.ln_edge_rows(9, width, g, dt)
    gamma, beta = 1 + 0.1 * torch.randn(width, generator=g), 0.1 * torch.randn(width, generator=g)
    u = OB.FMT[dt].u_out
    y, mean, rstd = OB.ln_reference(x, gamma, beta, 1e-5)
    yb, mb, rb = OB.ln_bounds(x, gamma, beta, 1e-5, u)
    ey, em, er = _ln_emulate(x, gamma, beta, 1e-5)
    assert assert_close_elementwise(OB.rnd(ey.double(), dt), y, yb, "y") <= 1
    assert assert_close_elementwise(em, mean, mb, "mean") <= 1 and assert_close_elementwise(er, rstd, rb, "rstd") <= 1
    assert abs(rstd[2].item() - 1e-5 ** -0.5) < 1e-9 and torch.equal(y[2], beta.double())
    _, _, rstd0 = OB.ln_reference(x, gamma, beta, 2e-5)
    assert ((rstd0 - rstd).abs() > rb)[2].item()
    wrong_mean = x.sum(-1) / (width + 1)
    assert ((wrong_mean - mean).abs() > mb)[1].item()
    # backward on the saved statistics: fp32 arithmetic in the kernel's order is inside on every row, the constant one included
    dy = OB.rnd(torch.randn(9, width, generator=g).double(), dt)
    dx, dx_e, _, dgam, dgam_b, dbet, dbet_b = OB.ln_bwd_reference(dy, x, gamma, em, er)
    xh = (x.float() - em[:, None]) * er[:, None]
    gg = dy.float() * gamma.float()
    c1, c2 = gg.sum(-1, keepdim=True) / width, (gg * xh).sum(-1, keepdim=True) / width
    edx = er[:, None] * (gg - c1 - xh * c2)
    assert assert_close_elementwise(OB.rnd(edx.double(), dt), dx, OB.SLACK * (dx_e + u * dx.abs()), "dx") <= 1
    assert assert_close_elementwise((dy.float() * xh).sum(0), dgam, dgam_b, "dgamma") <= 1 and assert_close_elementwise(dy.float().sum(0), dbet, dbet_b, "dbeta") <= 1
