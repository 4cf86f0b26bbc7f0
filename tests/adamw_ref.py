"""fp64 reference and per-element bounds of the fused AdamW (include/mmhip.h mmhip_adamw / mmhip_adamw_rows; csrc/heads.hip adamw_kernel,
adamw_rows_kernel), an fp32 emulation in the kernels' order and four wrong variants (pure torch, any device: tests/test_adamw_bounds_cpu.py checks
the bounds, tests/test_gpu_ops_adamw.py the kernels).

    ge = g grad_scale,  p1 = p (1 - lr wd),  m' = m + (1 - beta1)(ge - m),  v' = v beta2 + (1 - beta2) ge^2,
    p' = p1 - (lr / bc1) m' / (sqrt(v') / bc2s + eps),       bc1 = float(1 - beta1^step), bc2s = float(sqrt(1 - beta2^step)) formed in double on the host

The hyper-parameters are floats; the reference takes them as those floats and bc1 / bc2s exactly as csrc/mmhip_host.h adamw_args rounds them.
Constants: u = U_32; uf = SLACK u for one sqrtf or one division.  First-order terms, every one a rounding point of the kernel; the sum times SLACK.
    ge           e_ge = u |ge|
    m'           d = ge - m: e_ge + u |d|;  t = (1 - beta1) d: (1 - beta1)(e_ge + u |d|) + u |t|;  the add: + u |m'|       (1 - beta is exact for beta in [1/2, 1])
    v'           v beta2: u v beta2;  (1 - beta2) ge ge: (1 - beta2)(2 |ge| e_ge + 2 u ge^2);  the add: + u v'
    s = sqrt(v') e_v / (2 s) + uf s              (v' = 0 only where v = ge = 0: exact)
    q = s / bc2s e_s / bc2s + uf q;   den = q + eps: e_q + u den
    r = m' / den e_m / den + |r| e_den / den + uf |r|
    upd          step = lr / bc1 (uf);  step r: step e_r + |upd| (uf + u)
    p1           decay = fl(1 - fl(lr wd)): u lr wd + u absolute;  the product: u |p1|          (covers decay == 1.0f for lr wd < 2^-24)
    p'           e_p1 + e_upd + u |p'|
A fused multiply-add in place of a product and a sum drops one of these roundings and adds none."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from op_bounds import SLACK, U_32

U, UF = U_32, SLACK * U_32
f32 = lambda x: float(np.float32(x))

NS = [1, 3, 4, 5, 1027]
STEPS = [1, 2, 1000]
GRAD_SCALES = [1.0, 0.5]
# (lr, weight_decay): no decay; a decay a wrong order of operations shows under; the reference's defaults, where 1 - lr wd rounds to 1.0f
LR_WD = [(1e-3, 0.0), (1e-3, 0.01), (1e-5, 0.00025)]
ROW_WIDTHS = [4, 252, 256, 260, 768]
ROW_STATES = [0, 1, 2, 3, 3, 0, 1]          # seven rows: not a multiple of the four a workgroup takes, every state
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
BIG_N = 16384 * 1024 + 1024 + 3             # the smallest n at which adamw_kernel's grid-stride loop runs twice (16384 workgroups of 256 four-vectors)
VARIANTS = ("decay_after", "bc_step_minus_1", "eps_in_sqrt", "grad_scale_not_in_v")


def hyper(lr, wd, step, gs, beta1=BETA1, beta2=BETA2, eps=EPS):
    b1, b2 = f32(beta1), f32(beta2)
    return SimpleNamespace(lr=f32(lr), wd=f32(wd), b1=b1, b2=b2, eps=f32(eps), step=step, gs=f32(gs),
                           bc1=f32(1.0 - b1 ** step), bc2s=f32(math.sqrt(1.0 - b2 ** step)))


def applies(variant, h):
    """whether a wrong variant computes something else than the kernel at these hyper-parameters"""
    if variant == "decay_after":
        return f32(1.0 - f32(h.lr * h.wd)) != 1.0
    if variant == "bc_step_minus_1":
        return True
    if variant == "grad_scale_not_in_v":
        return h.gs != 1.0
    return True


def make_state(n, seed=0, device="cpu"):
    """p over four decades, a gradient with a few exact zeros, non-zero moments, v from 1e-16 to 1 (eps decides some denominators and not others)"""
    g_ = torch.Generator(device="cpu").manual_seed(1000 + n + seed)
    r = lambda: torch.randn(n, generator=g_)
    p = r() * 10.0 ** (-4 * torch.rand(n, generator=g_))
    g = r() * 10.0 ** (-3 * torch.rand(n, generator=g_))
    g[3::7] = 0.0
    m = 0.1 * r()
    v = 10.0 ** (-16 * torch.rand(n, generator=g_))
    # element 0 (all there is at n = 1): a small parameter, a gradient of 1e-3 and a second moment of 1e-12, so that eps, the bias corrections, the
    # decay's place and grad_scale each move it by far more than a rounding
    p[0], g[0], m[0], v[0] = 1.5e-3, -1.25e-3, 0.07, 1e-12
    return tuple(t.float().contiguous().to(device) for t in (p, g, m, v))


def make_state_on(n, device):
    """the same kind of state drawn on `device` (the one large case)"""
    g_ = torch.Generator(device=device).manual_seed(5)
    r = lambda f: f(n, generator=g_, device=device)
    p = r(torch.randn) * 10.0 ** (-4 * r(torch.rand))
    g = r(torch.randn) * 10.0 ** (-3 * r(torch.rand))
    m = 0.1 * r(torch.randn)
    v = 10.0 ** (-16 * r(torch.rand))
    return p, g, m, v


def reference(p, g, m, v, h, variant=None):
    """(p', m', v') in fp64 and their bounds; variant: one of VARIANTS (bounds are those of the right formula)"""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    omb1, omb2 = 1.0 - h.b1, 1.0 - h.b2
    bc1, bc2s = h.bc1, h.bc2s
    if variant == "bc_step_minus_1":
        bc1, bc2s = f32(1.0 - h.b1 ** (h.step - 1)), f32(math.sqrt(1.0 - h.b2 ** (h.step - 1)))
    ge = g * h.gs
    gv = g if variant == "grad_scale_not_in_v" else ge
    d = ge - m
    t = omb1 * d
    m1 = m + t
    v1 = v * h.b2 + omb2 * gv * gv
    s = torch.sqrt(v1 / bc2s ** 2 + h.eps) if variant == "eps_in_sqrt" else None
    s0 = torch.sqrt(v1)
    q = s0 / bc2s if bc2s else s0 / 0.0
    den = s if variant == "eps_in_sqrt" else q + h.eps
    r = m1 / den
    step = h.lr / bc1 if bc1 else float("inf")
    upd = step * r
    decay = 1.0 - h.lr * h.wd
    p1 = p * decay
    p2 = (p - upd) * decay if variant == "decay_after" else p1 - upd
    if variant is not None:
        return p2, m1, v1
    e_ge = U * ge.abs()
    e_m = omb1 * (e_ge + U * d.abs()) + U * t.abs() + U * m1.abs()
    e_v = U * v * h.b2 + omb2 * (2 * ge.abs() * e_ge + 2 * U * ge * ge) + U * v1
    e_s = torch.where(s0 > 0, e_v / (2 * s0.clamp_min(1e-300)), torch.zeros_like(s0)) + UF * s0
    e_q = e_s / bc2s + UF * q
    e_den = e_q + U * den
    e_r = e_m / den + r.abs() * e_den / den + UF * r.abs()
    e_upd = step * e_r + upd.abs() * (UF + U)
    e_p1 = p.abs() * (U * h.lr * h.wd + U) + U * p1.abs()
    e_p = e_p1 + e_upd + U * p2.abs()
    return (p2, m1, v1), (SLACK * e_p, SLACK * e_m, SLACK * e_v)


def emulate(p, g, m, v, h):
    """fp32, the kernels' order of operations (products and sums rounded one by one)"""
    F = lambda x: torch.tensor(x, dtype=torch.float32, device=p.device)
    p, g, m, v = (t.float() for t in (p, g, m, v))
    omb1, omb2 = F(1.0) - F(h.b1), F(1.0) - F(h.b2)
    decay, step = F(1.0) - F(h.lr) * F(h.wd), F(h.lr) / F(h.bc1)
    ge = g * F(h.gs)
    p = p * decay
    m = m + omb1 * (ge - m)
    v = v * F(h.b2) + omb2 * ge * ge
    den = torch.sqrt(v) / F(h.bc2s) + F(h.eps)
    return p - step * (m / den), m, v


def rows_state(width, seed=0):
    """[rows, width] p / g / m / v and the state bytes: rows without ROW_HAS_MOMENTS hold zero moments (the entry points' contract); the gradient of
    rows without ROW_HAS_GRAD is NOT zero here -- the kernel must neither read nor clear it"""
    rows = len(ROW_STATES)
    p, g, m, v = (t.view(rows, width) for t in make_state(rows * width, seed=width + seed))
    st = torch.tensor(ROW_STATES, dtype=torch.uint8)
    m[(st & 2) == 0] = 0.0
    v[(st & 2) == 0] = 0.0
    return p, g, m, v, st


def rows_reference(p, g, m, v, st, h, zero_grad):
    """what mmhip_adamw_rows leaves: (p', m', v') with bounds over rows that are updated (g read as 0 without ROW_HAS_GRAD), the state bytes, the
    gradient buffer; rows of state 0 are returned separately as the exact fp32 product p * fl(1 - fl(lr wd)), moments untouched"""
    has_g = ((st & 1) != 0)[:, None]
    g_eff = torch.where(has_g, g, torch.zeros_like(g))
    ref, bound = reference(p, g_eff, m, v, h)
    decay32 = torch.tensor(1.0, dtype=torch.float32) - torch.tensor(h.lr, dtype=torch.float32) * torch.tensor(h.wd, dtype=torch.float32)
    idle = st == 0
    exact_p = p.float() * decay32
    st_after = torch.where(idle, st, (2 | ((st & 1) if not zero_grad else torch.zeros_like(st))).to(torch.uint8))
    g_after = torch.where(has_g & bool(zero_grad), torch.zeros_like(g), g)
    return ref, bound, idle, exact_p, st_after, g_after
