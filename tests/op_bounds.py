"""fp64 references of the attention / quick-GELU / LayerNorm / GEMM (NT epilogues, TN, column sums) operators and the per-element error bounds the op tests hold the HIP kernels to
(pure torch on the CPU: tests/test_op_bounds_cpu.py checks the bounds themselves, the -m gpu modules check the kernels against them).

Every bound is a sum of named terms read off the kernels' rounding points, from four constants only:
    U_BF16 = 2^-8, U_F16 = 2^-11, U_32 = 2^-24 (unit roundoffs), U_PAIR = 2^-16 (a plane pair x = hi + lo carries 16 significant bits)
and one overall factor SLACK = 2 for v_exp_f32 / v_rcp_f32 / v_log_f32 (about an ulp each).  Nothing here is tuned to what a kernel returns.

Rounding model per dtype (`FMT`):
    prod(K)  relative error of one matrix product on (|A| |B|^T): K * U_32 of fp32 accumulation; the parity forms ("x3", "pair") add what the three
             products lose -- each operand is read as hi + lo and the lo.lo product is left out; where the operands are tensors the test knows this
             is computed from their actual parts (split_err), where the kernel forms one of them (P, dS) from U_PAIR / U_BF16 (split_err_w);
    u_p      rounding of P / dS to the MFMA operand type (16-bit kernels; the parity kernels split them inside the product: counted in prod);
    u_out    rounding of the stored result;  u_in  rounding of a stored input of the same kind (ctx as the backward reads it).
"alu" is the parity mode's fp32 vector-ALU fallback (csrc/x3.hip attn_*_f32*_kernel): fp32 everywhere, no split.
"""
import math
from collections import namedtuple

import torch

U_BF16, U_F16, U_32, U_PAIR = 2.0 ** -8, 2.0 ** -11, 2.0 ** -24, 2.0 ** -16
SLACK = 2.0
Fmt = namedtuple("Fmt", "name u_p u_out u_in split")
FMT = {"bf16": Fmt("bf16", U_BF16, U_BF16, U_BF16, 0.0), "f16": Fmt("f16", U_F16, U_F16, U_F16, 0.0),
       "x3": Fmt("x3", 0.0, U_32, U_32, 3 * U_PAIR), "pair": Fmt("pair", 0.0, U_PAIR, U_PAIR, 3 * U_PAIR),
       "alu": Fmt("alu", 0.0, U_32, U_32, 0.0)}


def prod(fmt, K):
    return fmt.split + K * U_32


def split_pair(x):
    """hi = bf16(x), lo = bf16(x - hi) of an fp32 tensor (csrc/mmhip_common.h split8, X3IO<true>::store4)"""
    x = x.float()
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def pair_hi_is_nearest(hi, lo):
    """the property the one-product readers of a plane pair rely on: the hi plane alone is the value rounded to bf16.  hi + lo is exact in fp32
    (two 8-bit significands at most 2^-8 apart), so "hi is a nearest bf16 of hi + lo" is checked exactly: |v - hi| <= |v - bf16(v)|.  Plain
    hi == bf16(hi + lo) is NOT implied by hi = bf16(x), lo = bf16(x - hi): when x - hi lies just under half an ulp of hi, lo rounds up to exactly
    half an ulp, hi + lo is a tie and round-to-even may pick hi's neighbour (about one element in a thousand); the inequality admits exactly those ties."""
    v = hi.float() + lo.float()
    return ((v - hi.float()).abs() <= (v - v.to(torch.bfloat16).float()).abs())


def rnd(x, name):
    """x (fp64) as the format stores / reads it, back in fp64"""
    if name == "bf16":
        return x.to(torch.bfloat16).double()
    if name == "f16":
        return x.to(torch.float16).double()
    if name in ("x3", "alu"):
        return x.float().double()
    hi, lo = split_pair(x)
    return hi.double() + lo.double()


def operand(x, name):
    """x (fp64) as a matrix-core operand of the format's products: exact for 16-bit values, hi + lo for the parity forms, fp32 on the ALUs"""
    return rnd(x, "pair") if name in ("x3", "pair") else rnd(x, name)


AttnRef = namedtuple("AttnRef", "q k v s live lse p a ks ctx dO dq dk dv")


def attn_reference(qkv, maskbias, posts, S, heads, keep=None, scale=1.0, dctx=None, score_scale=0.125, drop_last_key_of=None):
    """fp64 attention on `qkv` [posts*S, 3*heads*64] (already rounded to what the kernel reads).  keep: bool [posts, heads, S, S] or None.
    dq / dk / dv come from autograd.  drop_last_key_of = (post, head): that post's last live key is left out (the off-by-one reference)."""
    H = heads * 64
    x = qkv.double().view(posts, S, 3, heads, 64).clone().requires_grad_(dctx is not None)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) * score_scale
    live = torch.ones(posts, 1, 1, S, dtype=torch.bool)
    if maskbias is not None:
        s = s + maskbias.double().view(posts, 1, 1, S)
        live = torch.isfinite(maskbias.double()).view(posts, 1, 1, S)
    if drop_last_key_of is not None:
        pp, hh = drop_last_key_of
        last = int(live[pp, 0, 0].nonzero().max())
        kill = torch.zeros_like(s)
        kill[pp, hh, :, last] = float("-inf")
        s = s + kill
    lse = torch.logsumexp(s, dim=-1)
    p = torch.softmax(s, dim=-1)
    ks = torch.ones_like(p) if keep is None else keep.view_as(p).double() * scale
    a = p * ks
    o = a @ v
    dq = dk = dv = dO = None
    if dctx is not None:
        dO = dctx.double().view(posts, S, heads, 64).permute(0, 2, 1, 3)
        (o * dO).sum().backward()
        g = x.grad.permute(2, 0, 3, 1, 4)          # [3, posts, heads, S, 64]
        dq, dk, dv = g[0], g[1], g[2]
    d = lambda t: None if t is None else t.detach()
    return AttnRef(d(q), d(k), d(v), d(s), live.expand_as(s), d(lse), d(p), d(a), ks, d(o), dO, dq, dk, dv)


def to_rows(t):
    """[posts, heads, S, 64] -> [posts*S, heads*64] (the layout of ctx and of the q / k / v column blocks)"""
    P, Hh, S, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(P * S, Hh * D)


def _parts(x):
    """|x - hi - lo| and |lo| of x as the parity products read it (both 0 for a plane-pair input's residual: hi + lo is the value)"""
    hi, lo = split_pair(x)
    return (x.double() - hi.double() - lo.double()).abs(), lo.double().abs()


def split_err(fmt, A, Bt):
    """what three bf16 products lose on A @ Bt^T when BOTH operands are tensors the test knows (Q, K, V, dO, GEMM operands): read from the data, not
    from a worst case --  |A - hi - lo| |B| + |A| |B - hi - lo|  [what the pairs do not carry]  +  |lo_A| |lo_B|  [the product left out]"""
    if not fmt.split:
        return 0.0
    T = lambda t: t.transpose(-1, -2)
    ra, la = _parts(A)
    rb, lb = _parts(Bt)
    return ra @ T(Bt.abs()) + A.abs() @ T(rb) + la @ T(lb)


def split_err_w(fmt, W, X):
    """the same for W @ X with W >= 0 a quantity the KERNEL forms and splits (P, |dS|): its parts by their worst case, U_PAIR W and U_BF16 W, X's from the data"""
    if not fmt.split:
        return 0.0
    rx, lx = _parts(X)
    return U_PAIR * (W @ X.abs()) + W @ rx + U_BF16 * (W @ lx)


def _kdepth(fmt, K=64):
    """fp32 roundings behind one 64-deep dot product: the ALU kernels' dot64 keeps four partial sums of 16 fused multiply-adds and adds them in two
    steps (18); the matrix cores are charged the full K"""
    return 18 if fmt.name == "alu" else K


def _score_err(r, fmt, score_scale=0.125):
    """absolute error of a score as the soft-max sees it:  score_scale * (split_err(Q, K) + kdepth U_32 |q| |k|^T)  [the Q K^T product, kept in fp32: the
    16-bit kernels do not round it]  +  4 U_32 (|s| + |row max|)  [scale, bias add, max subtraction, the exponent's argument in fp32];  0 on masked keys"""
    qk = r.q.abs() @ r.k.abs().transpose(-1, -2)
    s0 = torch.where(r.live, r.s, torch.zeros_like(r.s))
    m = torch.where(r.live, r.s, torch.full_like(r.s, float("-inf"))).amax(-1, keepdim=True)
    e = score_scale * (split_err(fmt, r.q, r.k) + _kdepth(fmt) * U_32 * qk) + 4 * U_32 * (s0.abs() + m.abs())
    return torch.where(r.live, e, torch.zeros_like(e)), m.squeeze(-1)


def _acc(S):
    """fp32 steps behind one output element of a product over S keys: S accumulations + the rescale of the running sums per 32-key tile + the
    dropout scale and the final normalisation"""
    return S + 2 * ((S + 31) // 32) + 2


def attn_fwd_bounds(r, dt, S):
    """ctx:  2 E_i (A|V|)  [score error through the soft-max: |d p_ij| <= 2 E_i p_ij, E_i = the row's largest score error]
           + u_p (A|V|)    [P rounded to the operand type before P.V]
           + split_err_w(A, V) + acc(S) U_32 (A|V|)   [the P.V product]
           + u_out |ctx|   [the stored result];    A = P * keep * scale, all times SLACK.
    lse:   E_i + acc(S) U_32  [the fp32 sum of the exponentials]  + 4 U_32 (|lse| + |row max|)  [log, unit change, the final add], times SLACK."""
    fmt = FMT[dt]
    e, m = _score_err(r, fmt)
    E = e.amax(-1)
    av = r.a @ r.v.abs()
    ctx_b = SLACK * ((2 * E.unsqueeze(-1) + fmt.u_p + _acc(S) * U_32) * av + split_err_w(fmt, r.a, r.v) + fmt.u_out * r.ctx.abs())
    lse_b = SLACK * (E + _acc(S) * U_32 + 4 * U_32 * (r.lse.abs() + m.abs()))
    return ctx_b, lse_b


def attn_bwd_bounds(r, dt, S, score_scale=0.125, ctx_err=None, lse_err=None):
    """The backward recomputes p = exp(s - lse) (relative error rp = score error + 4 U_32 |lse|), dP = dO V^T (split_err(dO, V) + kdepth U_32 |dO||V|^T,
    times the dropout scale), D = sum_d ctx dO (u_in + 64 U_32 on sum |ctx||dO|: ctx is read as stored), dS = p (dP keep scale - D) / 8, then rounds P
    and dS to the operand type (u_p) for  dV = A^T dO,  dK = dS^T Q,  dQ = dS K  and rounds the results (u_out):
        d(dS) = (rp p |dP' - D| + p (d dP + d D)) / 8 + (u_p + 4 U_32) |dS|
        dV:  ((rp + u_p) A)^T |dO| + split_err_w(A^T, dO) + acc(S) U_32 A^T |dO| + u_out |dV|
        dK:  d(dS)^T |Q| + split_err_w(|dS|^T, Q) + acc(S) U_32 |dS|^T |Q| + u_out |dK|        dQ: the same with dS, K
    all times SLACK.  A masked key has p = 0 exactly: its dK / dV bounds are 0, i.e. exact zeros are required.
    ctx_err / lse_err: when the backward is fed a forward's OWN ctx and lse (the composite blocks) instead of the reference's, their forward bounds
    enter as d D += sum_d ctx_err |dO| and rp += lse_err."""
    fmt = FMT[dt]
    e, _ = _score_err(r, fmt)
    rp = e + 4 * U_32 * r.lse.abs().unsqueeze(-1)
    if lse_err is not None:
        rp = rp + lse_err.unsqueeze(-1)
    dOa, T = r.dO.abs(), (lambda t: t.transpose(-1, -2))
    dP = r.dO @ T(r.v)
    d_dP = (split_err(fmt, r.dO, r.v) + _kdepth(fmt) * U_32 * (dOa @ T(r.v.abs()))) * r.ks
    D = (r.ctx * r.dO).sum(-1, keepdim=True)
    d_D = (fmt.u_in + 64 * U_32) * (r.ctx.abs() * dOa).sum(-1, keepdim=True)
    if ctx_err is not None:
        d_D = d_D + (ctx_err * dOa).sum(-1, keepdim=True)
    inner = dP * r.ks - D
    dS = r.p * inner * score_scale
    d_dS = score_scale * (rp * r.p * inner.abs() + r.p * (d_dP + d_D)) + (fmt.u_p + 4 * U_32) * dS.abs()
    acc = _acc(S) * U_32
    dv_b = SLACK * (T((rp + fmt.u_p) * r.a) @ dOa + split_err_w(fmt, T(r.a), r.dO) + acc * (T(r.a) @ dOa) + fmt.u_out * r.dv.abs())
    dk_b = SLACK * (T(d_dS) @ r.q.abs() + split_err_w(fmt, T(dS.abs()), r.q) + acc * (T(dS.abs()) @ r.q.abs()) + fmt.u_out * r.dk.abs())
    dq_b = SLACK * (d_dS @ r.k.abs() + split_err_w(fmt, dS.abs(), r.k) + acc * (dS.abs() @ r.k.abs()) + fmt.u_out * r.dq.abs())
    return dq_b, dk_b, dv_b


def attn_emulate(r, dt, score_scale=0.125):
    """the reference with the kernels' casts inserted: operands as the matrix cores read them (three products for the parity forms), P and dS
    rounded to the operand type, ctx rounded as stored and read back by the backward, results rounded.  Returns ctx, lse, dq, dk, dv."""
    fmt = FMT[dt]
    T = lambda t: t.transpose(-1, -2)

    def mm(a, b):
        if not fmt.split:
            return (a @ b).float().double()
        ah, al = split_pair(a)
        bh, bl = split_pair(b)
        return (al.double() @ bh.double() + ah.double() @ bl.double() + ah.double() @ bh.double()).float().double()

    rp_ = (lambda t: rnd(t, dt)) if fmt.u_p else (lambda t: t.float().double())
    s = mm(r.q, T(r.k)) * score_scale
    s = torch.where(r.live, s, torch.full_like(s, float("-inf")))
    m = s.amax(-1, keepdim=True)
    pt = torch.exp(s - m).float().double()
    l = pt.sum(-1, keepdim=True)
    ctx = rnd(mm(rp_(pt * r.ks), r.v) / l, dt)
    lse = (m + torch.log(l)).squeeze(-1).float().double()
    if r.dO is None:
        return ctx, lse, None, None, None
    ctx_in = rnd(r.ctx, dt)                      # the backward under test is fed the reference's ctx / lse, as stored
    lse_in = r.lse.float().double().unsqueeze(-1)
    p = torch.exp(s - lse_in).float().double()
    dP = mm(r.dO, T(r.v)) * r.ks
    D = (ctx_in * r.dO).sum(-1, keepdim=True).float().double()
    dS = (p * (dP - D) * score_scale).float().double()
    dv = rnd(mm(T(rp_(p * r.ks)), r.dO), dt)
    dk = rnd(mm(T(rp_(dS)), r.q), dt)
    dq = rnd(mm(rp_(dS), r.k), dt)
    return ctx, lse, dq, dk, dv


def attn_inputs(dt, posts, S, heads, masked, seed, with_dctx=False):
    """qkv (and d ctx) as fp64 values exactly representable in what the kernel reads, and the additive key mask.  Mask lengths: post 0 keeps all S
    keys, post 1 a single key, post 2 (if any) leaves at least one whole 32-key tile masked -- and for S >= 289 a whole 288-key chunk of the long
    parity kernel --, the rest are drawn."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    H = heads * 64
    name = "x3" if dt in ("x3", "alu") else dt
    qkv = rnd(torch.randn(posts * S, 3 * H, generator=g).double(), name)
    dctx = rnd(torch.randn(posts * S, H, generator=g).double(), name) if with_dctx else None
    maskbias = None
    if masked:
        lens = torch.randint(1, S + 1, (posts,), generator=g)
        lens[0] = S
        if posts > 1:
            lens[1] = 1
        if posts > 2:
            lens[2] = max(1, S - 288 - 5) if S >= 289 + 6 else max(1, S - 37)
        maskbias = torch.where(torch.arange(S)[None, :] < lens[:, None], 0.0, float("-inf")).float().contiguous()
    return qkv, dctx, maskbias


# ---------------------------------------------------------------------------------------------------------------- quick-GELU, LayerNorm pair
def qgelu_reference(x, c=1.702):
    x = x.double()
    return x / (1.0 + torch.exp(-c * x))


def qgelu_bound(x):
    """mm_qgelu(x) = x * rcp(1 + exp(-1.702 x)) in fp32 (csrc/mmhip_common.h).  With e = exp(-1.702 x), sigma = 1 / (1 + e):
        the product 1.702 x rounds (U_32 |1.702 x|: a RELATIVE error of that size on e), __expf itself (U_32 on e), the sum 1 + e (U_32), v_rcp
        (U_32), the product x * sigma (U_32);  d sigma / sigma = (e / (1 + e)) * (d e / e) for the first two.
        bound = |ref| * U_32 * (3 + (1 - sigma) * (1 + |1.702 x|)) * SLACK"""
    x = x.double()
    sig = 1.0 / (1.0 + torch.exp(-1.702 * x))
    return SLACK * qgelu_reference(x).abs() * U_32 * (3 + (1 - sig) * (1 + (1.702 * x).abs()))


def ln_reference(x, gamma, beta, eps):
    x = x.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean) * rstd * gamma.double() + beta.double(), mean.squeeze(-1), rstd.squeeze(-1)


def ln_bounds(x, gamma, beta, eps, u_out):
    """y = (x - mean) rstd gamma + beta on fp32 rows of width W, one wave per row: a lane adds its 4 ceil(W / 256) elements, six shuffle steps add the
    lanes -- n = 4 ceil(W / 256) + 6 roundings per sum.  mean carries n U_32 mean|x|, rstd a relative n U_32 (sum of squares)
    + 2 U_32 (rsqrt, eps add);  per element  |gamma| rstd d_mean + |y - beta| (d rstd / rstd + 3 U_32)  [subtraction, two products]
    + U_32 |y| [the add] + u_out |y| [the store], times SLACK.  mean / rstd outputs: their own terms + U_32 for the store."""
    x = x.double()
    W = x.shape[-1]
    y, mean, rstd = ln_reference(x, gamma, beta, eps)
    n = 4 * ((W + 255) // 256) + 6
    d_mean = n * U_32 * x.abs().mean(-1, keepdim=True)
    # d var = 2 d_mean mean|x - mean| (two-pass variance), d rstd / rstd = d var rstd^2 / 2
    rel_rstd = (n + 2) * U_32 + d_mean * (x - mean.unsqueeze(-1)).abs().mean(-1, keepdim=True) * rstd.unsqueeze(-1) ** 2
    yb = SLACK * (gamma.double().abs() * rstd.unsqueeze(-1) * d_mean + (y - beta.double()).abs() * (rel_rstd + 3 * U_32) + (U_32 + u_out) * y.abs())
    mean_b = SLACK * (d_mean.squeeze(-1) + U_32 * mean.abs())
    rstd_b = SLACK * (rel_rstd.squeeze(-1) + U_32) * rstd
    return yb, mean_b, rstd_b


def ln_edge_rows(rows, width, g, dt):
    """the LayerNorm inputs of the op tests: ordinary rows (spread 2, mean 0.3), every fourth row with mean 1e3 and unit spread, row 2 (if any) constant"""
    x = torch.randn(rows, width, generator=g) * 2 + 0.3
    x[1::4] = torch.randn(len(range(1, rows, 4)), width, generator=g) + 1e3
    if rows > 2:
        x[2] = 0.3
    return rnd(x.double(), dt)


# ---------------------------------------------------------------------------------------------------------------- GEMM epilogues, LayerNorm backward
def erf_gelu(v):
    return v * 0.5 * torch.erfc(-v / math.sqrt(2.0))


def erf_gelu_grad(u):
    return 0.5 * torch.erfc(-u / math.sqrt(2.0)) + u * torch.exp(-u * u / 2) / math.sqrt(2 * math.pi)


GELU_ABS, GELU_GRAD_ABS = 4.8e-7, 1.3e-6          # mm_gelu / mm_gelu_grad2: absolute error by construction (csrc/mmhip_common.h, tests/test_gpu_ops.py)


NTProducts = namedtuple("NTProducts", "v ab se K")


def gemm_nt_products(A, B, dt):
    """step one of gemm_nt_reference, computed once per (A, B) and shared by every epilogue variant of that pair: the fp64 product A B^T, |A| |B|^T
    and split_err(A, B) (0 for the 16-bit formats).  Works on whatever device A and B live on."""
    A, B = A.double(), B.double()
    return NTProducts(A @ B.t(), A.abs() @ B.abs().t(), split_err(FMT[dt], A, B), A.shape[-1])


def gemm_nt_reference(A, B, dt, bias=None, act=0, mulg=None, keep=None, scale=1.0, resid=None, out="t", products=None):
    """fp64 epilogue(A B^T) of mmhip_op_gemm_nt on the values the kernel reads, with its per-element bound:
        acc:   split_err(A, B) + K U_32 |A| |B|^T   [the product]  + U_32 |acc + bias|  [bias add]
        act 1: GELU_ABS + |gelu'| <= 1.13 times the accumulator's error + U_32 |.|;   aux (the pre-activation) = acc error + u_out |pre|
        mulg:  times gelu'(u): (acc error) |gelu'(u)| + GELU_GRAD_ABS |acc| + U_32 |.|
        dropout: times keep * scale (+ U_32);  residual: + U_32 |sum|;  store: u_out |result|;    all times SLACK.
    out = "f32": the result is stored as fp32 (u_out = U_32); with no bias and no activation that is the bare accumulator against K U_32 |A| |B|^T.
    products: gemm_nt_products(A, B, dt) when several variants share one (A, B) -- A and B are then not touched.
    Returns (C, C bound, pre, pre bound)."""
    fmt = FMT[dt]
    pr = products if products is not None else gemm_nt_products(A, B, dt)
    v = pr.v
    e = pr.se + pr.K * U_32 * pr.ab
    if bias is not None:
        v = v + bias.double()
        e = e + U_32 * v.abs()
    u_out = U_32 if out == "f32" else fmt.u_out
    pre, pre_b = v, SLACK * (e + u_out * v.abs())
    if act == 1:
        v, e = erf_gelu(v), 1.13 * e + GELU_ABS + U_32 * erf_gelu(v).abs()
    if act == 2:          # tanhf: |tanh'| <= 1, a few ulp of its own
        v, e = torch.tanh(v), e + 4 * U_32 * torch.tanh(v).abs()
    if mulg is not None:
        gp = erf_gelu_grad(mulg.double())
        e = e * gp.abs() + GELU_GRAD_ABS * v.abs() + U_32 * (v * gp).abs()
        v = v * gp
    if keep is not None:
        ks = keep.double() * scale
        v, e = v * ks, (e + U_32 * v.abs()) * ks
    if resid is not None:
        v = v + resid.double()
        e = e + U_32 * v.abs()
    return v, SLACK * (e + u_out * v.abs()), pre, pre_b


def gemm_tn_reference(A, B, dt, C0=None, colsum0=None):
    """fp64  C = C0 + A^T B  (A [M, Nn], B [M, Nc]: the weight gradient dW = dY^T X) and the column sums  cs = colsum0 + sum_r A[r]  of
    mmhip_op_gemm_tn / _group on the values the kernels read, each with its per-element bound:
        C:   split_err(A^T, B^T)   [parity mode: what the three bf16 products lose; 0 for the 16-bit formats, whose operands enter the matrix cores exactly]
           + M U_32 |A|^T |B|      [fp32 accumulation of M products in any order: MFMA chains, partial sums, atomics]
           + U_32 |C|              [the store: alpha * acc rounded to fp32]   + U_32 |C| once more with C0 [the accumulate add]
        cs:  sum_r |A - hi - lo|   [parity mode: the sums are taken over the hi and lo planes, the residual is not carried; 0 otherwise]
           + M U_32 sum_r |A|      [fp32 accumulation]  + U_32 |cs| [store]  + U_32 |cs| with colsum0 [accumulate add]
    all times SLACK.  Returns (C, C bound, cs, cs bound)."""
    fmt = FMT[dt]
    A, B = A.double(), B.double()
    M = A.shape[0]
    At, Bt = A.t(), B.t()
    C = At @ B
    e = split_err(fmt, At, Bt) + M * U_32 * (At.abs() @ B.abs())
    cs = A.sum(0)
    ce = M * U_32 * A.abs().sum(0)
    if fmt.split:
        ce = ce + _parts(A)[0].sum(0)
    if C0 is not None:
        C = C + C0.double()
        e = e + U_32 * C.abs()
    if colsum0 is not None:
        cs = cs + colsum0.double()
        ce = ce + U_32 * cs.abs()
    return C, SLACK * (e + U_32 * C.abs()), cs, SLACK * (ce + U_32 * cs.abs())


def colsum_reference(x, out0=None):
    """fp64  out0 + sum_r x[r]  of mmhip_op_colsum (csrc/rowops.hip colsum_kernel: fp32 partial sums per 64-row chunk, one atomic add per chunk into out --
    the kernel ADDS to what out holds) with the bound  rows U_32 (|out0| + sum_r |x|)  [every add, in any order, rounds a running sum no larger than
    that], times SLACK.  The input is read exactly (16-bit and fp32 values are fp32 values)."""
    x = x.double()
    ref, mag = x.sum(0), x.abs().sum(0)
    if out0 is not None:
        ref, mag = ref + out0.double(), mag + out0.double().abs()
    return ref, SLACK * x.shape[0] * U_32 * mag


def ln_bwd_reference(dy, x, gamma, mean, rstd, keep=None, scale=1.0):
    """LayerNorm backward on the saved row statistics (fp64): dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dy gamma;  dgamma = sum_r dy xhat,
    dbeta = sum_r dy;  dd = dx * keep * scale.  Bounds (fp32 rows, one sum = n = 4 ceil(W / 256) + 6 roundings as in ln_bounds):
        xhat, g: 2 U_32 each;  m1 = mean(g): n U_32 mean|g|;  m2 = mean(g xhat): (n + 5) U_32 mean|g xhat|
        dx: rstd (4 U_32 |g| + d m1 + |xhat| d m2 + 5 U_32 |xhat m2|) + 2 U_32 |dx| + u_out |dx|   (u_out added by the caller)
        dgamma / dbeta: (rows + 4) U_32 sum_r |dy xhat| resp. rows U_32 sum_r |dy|  (fp32 partial sums and atomics in any order)"""
    dy, x, gamma = dy.double(), x.double(), gamma.double()
    mean, rstd = mean.double().unsqueeze(-1), rstd.double().unsqueeze(-1)
    R, W = x.shape
    n = 4 * ((W + 255) // 256) + 6
    xhat = (x - mean) * rstd
    g = dy * gamma
    m1, m2 = g.mean(-1, keepdim=True), (g * xhat).mean(-1, keepdim=True)
    dx = rstd * (g - m1 - xhat * m2)
    d1 = n * U_32 * g.abs().mean(-1, keepdim=True)
    d2 = (n + 5) * U_32 * (g * xhat).abs().mean(-1, keepdim=True)
    dx_e = rstd * (4 * U_32 * g.abs() + d1 + xhat.abs() * d2 + 5 * U_32 * (xhat * m2).abs()) + 2 * U_32 * dx.abs()
    dgam, dbet = (dy * xhat).sum(0), dy.sum(0)
    dgam_b = SLACK * (R + 4) * U_32 * (dy * xhat).abs().sum(0)
    dbet_b = SLACK * R * U_32 * dy.abs().sum(0) + 1e-300
    dd = dx if keep is None else dx * keep.double() * scale
    return dx, dx_e, dd, dgam, dgam_b + 1e-300, dbet, dbet_b
