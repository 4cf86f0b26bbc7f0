"""fp64 reference and per-element bounds of the CLS-query fusion attention (include/mmhip.h mmhip_op_fusion_attn_fwd / _bwd; csrc/heads.hip
fusion_attn_fwd_kernel, fusion_attn_bwd_kernel: one workgroup of 8 waves per row bt, image tokens of post bt % B), an fp32 emulation and four wrong
variants (pure torch on the CPU: tests/test_fusion_attn_bounds_cpu.py checks the bounds, tests/test_gpu_ops_fusion_attn.py the kernels).

    fwd   s_j = scale qk . x_j,   p = softmax(s),   xbar = sum_j p_j x_j
    bwd   dp_j = dxbar . x_j,   ds_j = scale p_j (dp_j - sum_i p_i dp_i),   dqk = sum_j ds_j x_j          (prob as handed in: the reference's, as fp32)

The image tokens are read exactly (a 16-bit value is an fp32 value); everything else is fp32.
Constants: u = U_32, uf = SLACK u for one __expf / division, gamma(k) = k u / (1 - k u), TINY = 2^-126 (an exponential below the normal range).
    dot over H     a lane chains its 4 ceil(H / 256) multiply-adds, six shuffle steps add the lanes: gamma(D) |a| . |x|,  D = 4 ceil(H / 256) + 6
    s_j            d_j = scale gamma(D) |qk| . |x_j| + u |s_j|
    p_j            through the soft-max: p_j (d_j + sum_i p_i d_i);  arithmetic: r_j = uf + 2 u |s_j - max| for the exponential (the subtraction and
                   the scaling to base 2 round its argument), the sum over the workgroup (six shuffle steps, 8 waves: gamma(14)) carries the p-weighted
                   mean of the r_i, the division uf:  p_j (r_j + sum_i p_i r_i + gamma(14) + uf) + TINY
    xbar, dqk      a wave chains ceil(P / 8) multiply-adds, the 8 partial rows are added in sequence:  sum_j e_j |x_j| + gamma(ceil(P / 8) + 8) sum_j |w_j x_j|
    tsum           sum_i p_i dp_i: sum_i p_i e_dp_i + gamma(15) sum_i |p_i dp_i|
    ds_j           scale p_j (e_dp_j + e_tsum + u |dp_j - tsum|) + 2 u |ds_j|
The whole sum times SLACK."""
import math
from types import SimpleNamespace

import torch

from op_bounds import SLACK, U_32

U, UF = U_32, SLACK * U_32
TINY = 2.0 ** -126
BT_B = [(1, 1), (3, 3), (4, 2)]
SHAPES = [(P, 768) for P in (1, 3, 4, 5, 31, 33, 197, 512)] + [(P, H) for H in (4, 252, 256, 260, 1024) for P in (33, 197)]          # (P, H)
DTYPES = ("bf16", "f16", "x3")
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "x3": torch.float32}
VARIANTS = ("tokens_of_post_bt", "last_token_dropped", "no_scale_in_backward", "no_sum_p_dp")


def gamma(k):
    return k * U / (1.0 - k * U)


def make_inputs(dt, Bt, B, P, H, seed=0):
    """scores spread over about +-30 (without the max subtraction __expf would overflow); in rows 0 and 2 one token dominates; dxbar has mean 0.5"""
    g = torch.Generator().manual_seed(1009 * P + 13 * H + 7 * Bt + B + seed)
    xv = torch.randn(B, P, H, generator=g).to(TORCH_DT[dt])
    scale = 1.0 / math.sqrt(H)
    qk = 10.0 * torch.randn(Bt, H, generator=g)
    qk = (qk * (10.0 * math.sqrt(H) / qk.norm(dim=1, keepdim=True))).float()          # |qk| = 10 sqrt(H): a score is 10 x_j . (unit vector), whatever H

    def plant(bt, j, lead):
        """token j of row bt's post becomes a multiple of qk[bt] whose score leads every other token's by `lead` (the other scores do not move)"""
        X, q = xv[bt % B].double(), qk[bt].double()
        others = torch.cat([X[:j], X[j + 1:]]) @ q * scale
        xv[bt % B, j] = ((others.max() + lead) / (scale * (q @ q)) * q).to(xv.dtype)

    if P > 1:
        if Bt > 2:          # row 2: one token 30 ahead, all but alone in the soft-max
            plant(2, 12 % P, 30.0)
        # row 0 (all there is at Bt = 1): the LAST token, the one the clamp min(j0 + u, P - 1) repeats, leads by 3 -- it dominates, and the
        # runners-up still carry weight for the backward
        plant(0, P - 1, 3.0)
    dxbar = torch.randn(Bt, H, generator=g) + 0.5
    return SimpleNamespace(dt=dt, Bt=Bt, B=B, P=P, H=H, scale=float(torch.tensor(scale, dtype=torch.float32)), xv=xv.contiguous(), qk=qk.float().contiguous(),
                           dxbar=dxbar.float().contiguous())


def _tokens(c, variant=None):
    """[Bt, P, H] fp64: the tokens row bt reads"""
    post = torch.arange(c.Bt) % c.B
    if variant == "tokens_of_post_bt":          # (rows past B have no post of their own: they are given another one than bt % B)
        post = torch.where(torch.arange(c.Bt) < c.B, post, c.B - 1 - post)
    return c.xv.double()[post]


def fwd_reference(c, variant=None):
    X = _tokens(c, variant)
    q = c.qk.double()
    D = 4 * ((c.H + 255) // 256) + 6
    s = c.scale * torch.einsum("bh,bph->bp", q, X)
    if variant == "last_token_dropped":
        s = s.clone()
        s[:, -1] = -float("inf")
    p = torch.softmax(s, dim=1)
    xbar = torch.einsum("bp,bph->bh", p, X)
    ref = dict(prob=p, xbar=xbar)
    if variant is not None:
        return ref
    d = c.scale * gamma(D) * torch.einsum("bh,bph->bp", q.abs(), X.abs()) + U * s.abs()
    r = UF + 2 * U * (s - s.max(dim=1, keepdim=True).values).abs()
    e_p = p * (d + (p * d).sum(1, keepdim=True)) + p * (r + (p * r).sum(1, keepdim=True) + gamma(14) + UF) + TINY
    e_x = torch.einsum("bp,bph->bh", e_p, X.abs()) + gamma((c.P + 7) // 8 + 8) * torch.einsum("bp,bph->bh", p, X.abs())
    return ref, dict(prob=SLACK * e_p, xbar=SLACK * e_x)


def bwd_reference(c, prob, variant=None):
    """prob: fp32 [Bt, P] as the kernel is handed it"""
    X = _tokens(c, variant)
    p, dx = prob.double(), c.dxbar.double()
    D = 4 * ((c.H + 255) // 256) + 6
    dp = torch.einsum("bh,bph->bp", dx, X)
    pd = p * dp
    tsum = pd.sum(1, keepdim=True)
    if variant == "no_sum_p_dp":
        tsum = torch.zeros_like(tsum)
    ds = p * (dp - tsum) * (1.0 if variant == "no_scale_in_backward" else c.scale)
    dqk = torch.einsum("bp,bph->bh", ds, X)
    if variant is not None:
        return dict(dqk=dqk)
    e_dp = gamma(D) * torch.einsum("bh,bph->bp", dx.abs(), X.abs())
    e_t = (p * e_dp).sum(1, keepdim=True) + gamma(15) * pd.abs().sum(1, keepdim=True)
    e_ds = c.scale * p * (e_dp + e_t + U * (dp - tsum).abs()) + 2 * U * ds.abs()
    e = torch.einsum("bp,bph->bh", e_ds, X.abs()) + gamma((c.P + 7) // 8 + 8) * torch.einsum("bp,bph->bh", ds.abs(), X.abs())
    return dict(dqk=dqk), dict(dqk=SLACK * e)


def applies(variant, c):
    """(P = 1: the one weight is 1 and the backward's result 0 whatever the scale or the sum)"""
    return {"tokens_of_post_bt": c.Bt > c.B, "last_token_dropped": c.P > 1, "no_scale_in_backward": c.scale != 1.0 and c.P > 1, "no_sum_p_dp": c.P > 1}[variant]


def emulate(c, prob):
    """both directions in fp32"""
    X = c.xv.float()[torch.arange(c.Bt) % c.B]
    sc = torch.tensor(c.scale, dtype=torch.float32)
    s = torch.einsum("bh,bph->bp", c.qk, X) * sc
    e = torch.exp(s - s.max(dim=1, keepdim=True).values)
    p = e / e.sum(1, keepdim=True)
    out = dict(prob=p, xbar=torch.einsum("bp,bph->bh", p, X))
    dp = torch.einsum("bh,bph->bp", c.dxbar, X)
    tsum = (prob * dp).sum(1, keepdim=True)
    out["dqk"] = torch.einsum("bp,bph->bh", prob * (dp - tsum) * sc, X)
    return out
