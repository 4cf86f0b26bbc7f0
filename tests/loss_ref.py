"""fp64 reference and per-element bounds of the fused loss mix (include/mmhip.h mmhip_op_loss; csrc/heads.hip loss_kernel: one workgroup of 256 threads,
stride loops over up to 1024 posts), an fp32 emulation and five wrong variants (pure torch on the CPU: tests/test_loss_bounds_cpu.py checks the
bounds, tests/test_gpu_ops_loss.py the kernel).

    cls  = -(1 / B) sum_bc w_c y_bc (z_bc - lse_b),   d z_bc = w_cls (softmax(z)_bc wy_b - w_c y_bc) / B,  wy_b = sum_c w_c y_bc   (y = (float)onehot)
    itc  = (1 / 2B) sum_i (rowlse_i - S_ii) + (collse_i - S_ii),   d S_ij = w_itc (exp(S_ij - rowlse_i) + exp(S_ij - collse_j) - 2 [i = j]) / 2B
    itm  = (1 / B) sum_b lse(t_b) - t_b[y_b],   d t_bk = w_itm (softmax(t_b)_k - [y_b = k]) / B;      total = w_cls cls + w_itc itc + w_itm itm

Constants: u = U_32, uf = SLACK u for one __expf / __logf / division, gamma(k) = k u / (1 - k u).  First-order terms, SLACK entering
through uf alone as in tests/itc_ref.py:
    e = __expf(a - b): the subtraction and the scaling to base 2 round the argument, relative uf + 2 u |a - b|, plus the absolute error of b when b is a
        computed log-sum-exp, plus TINY = 2^-126 absolute (a result below the normal range may be flushed to 0)
    lse = mx + __logf(sum_k e_k): (sum_k e_k r_k + gamma(n) sum) / sum  +  uf log(sum)  +  u |lse|          (mx is exact; n terms added in sequence)
    a loss: every term's own error, plus gamma(depth) sum |term| for the thread's ceil(B / 256) n_per_row additions, the 6 shuffle steps, the 3 adds
        over the waves and the division -- all over the divisor
    gradients: ABSOLUTE in their parts -- p r_p (+ q r_q) for the exponentials, u per partial sum of the cancellation p + q - 2 or p wy - w y, and
        (u + uf) |d| for the final product and division.  On the ITC diagonal the parts cancel to near 0 and a relative bound would mean nothing.
    total: w e_term per term, plus gamma(3) sum |w term|."""
from types import SimpleNamespace

import numpy as np
import torch

from op_bounds import SLACK, U_32

U, UF = U_32, SLACK * U_32
TINY = 2.0 ** -126          # an exponential below the smallest normal fp32 may come out as 0: absolute, per __expf
BC = [(1, 3), (2, 3), (3, 3), (255, 3), (256, 3), (257, 3), (1024, 3), (257, 2), (257, 7), (3, 2), (3, 7)]
ITC_MODES = ("off", "logits", "global")
W_CLS, W_ITC, W_ITM = (float(np.float32(x)) for x in (0.9, 0.35, 0.2))
ITC_GLOBAL = float(np.float32(3.21875))
TIE_ROWS = (1, 5, 256)
MIN_GAP = 1e-3
VARIANTS = ("col_lse_over_row", "no_wy", "itc_over_B", "itm_label_flipped", "rows_from_256_skipped")


def gamma(k):
    return k * U / (1.0 - k * U)


def make_inputs(B, C, seed=0):
    g = torch.Generator().manual_seed(31 * B + C + seed)
    z = (torch.randn(B, C, generator=g) * (0.1 + 40 * torch.rand(B, 1, generator=g))).clamp(-80, 80).float()
    # top-two gap of every row at least MIN_GAP (n_correct is held to equality) ...
    top2 = z.double().topk(min(2, C), dim=1).values
    close = (top2[:, 0] - top2[:, -1]) < 2 * MIN_GAP
    z[close, 0] += 1.0
    # ... but for planted rows whose first and last columns hold the same maximum: the first index counts
    ties = [r for r in TIE_ROWS if r < B]
    for r in ties:
        z[r, 0] = z[r, C - 1] = z[r].max() + 0.5
    lab = torch.randint(0, C, (B,), generator=g)
    y = torch.zeros(B, C, dtype=torch.int64)
    y[torch.arange(B), lab] = 1
    for r in range(B):          # soft-target rows: two-hot, all-zero, one holding a 2
        if r % 8 == 1:
            y[r, (lab[r] + 1) % C] = 1
        elif r % 8 == 2:
            y[r] = 0
        elif r % 8 == 4:
            y[r, lab[r]] = 2
    cw = (0.5 + 0.75 * torch.arange(C)).float()
    S = (25 * torch.randn(B, B, generator=g)).clamp(-100, 100).float()
    idx = torch.arange(0, B, 3)
    S[idx, idx] = (S[idx].max(dim=1).values + 10).clamp(max=100.0)          # the diagonal dominates every third row (and mostly not its column)
    t = (5 * torch.randn(B, 2, generator=g)).float()
    lt = torch.randint(0, 2, (B,), generator=g)
    return SimpleNamespace(B=B, C=C, z=z, y=y, cw=cw, S=S, t=t, lt=lt, ties=ties)


def first_argmax(x):
    """index of the first maximum of every row (what the kernel's strict > keeps)"""
    n = x.shape[1]
    return torch.where(x == x.max(dim=1, keepdim=True).values, torch.arange(n)[None, :], n).min(dim=1).values


def n_correct(c):
    return int((first_argmax(c.z.double()) == first_argmax(c.y.double())).sum())


def _lse(x, dim):
    """log-sum-exp of fp32 values along dim as the kernel forms it, and its absolute error"""
    mx = x.max(dim=dim, keepdim=True).values
    d = x - mx
    e = torch.exp(d)
    s = e.sum(dim=dim, keepdim=True)
    n = x.shape[dim]
    e_s = (e * (UF + 2 * U * d.abs()) + TINY).sum(dim=dim, keepdim=True) + gamma(n) * s
    lse = mx + torch.log(s)
    return lse.squeeze(dim), (e_s / s + UF * torch.log(s) + U * lse.abs()).squeeze(dim)


def _depth(B, per_row):
    return ((B + 255) // 256) * per_row + 6 + 3 + 1


def reference(c, class_w, itc, itm, variant=None):
    """dict of fp64 outputs (loss [4], d_out_cls, d_logits, d_out_tim -- the latter two only when their term is on) and the dict of bounds.
    class_w: bool; itc: one of ITC_MODES; itm: bool.  variant: one of VARIANTS (the bounds stay those of the right formula)."""
    B, C = c.B, c.C
    live = torch.ones(B, dtype=torch.bool)
    if variant == "rows_from_256_skipped":
        live[256:] = False
    lv = live.double()
    z, y = c.z.double(), c.y.double()
    w = (c.cw.double() if class_w else torch.ones(C, dtype=torch.float64))[None, :]
    ref, b = {}, {}
    # ---- classification
    lse, e_lse = _lse(z, 1)
    dz = z - lse[:, None]
    t = w * y * dz
    e_t = (w * y).abs() * (e_lse[:, None] + U * dz.abs()) + 2 * U * t.abs()
    lc = -(t * lv[:, None]).sum() / B
    e_lc = (e_t.sum() + gamma(_depth(B, C)) * t.abs().sum()) / B
    wy = (w * y).sum(1, keepdim=True)
    e_wy = gamma(C + 1) * (w * y).abs().sum(1, keepdim=True)
    p = torch.exp(dz)
    rp = UF + 2 * U * dz.abs() + e_lse[:, None]
    a_, b_ = p * (1.0 if variant == "no_wy" else wy), w * y
    d = W_CLS * (a_ - b_) / B
    ref["d_out_cls"] = d * lv[:, None]
    b["d_out_cls"] = W_CLS / B * ((p * (rp + U) + TINY) * wy + p * e_wy + U * b_.abs() + U * (p * wy - b_).abs()) + (U + UF) * d.abs()
    # ---- ITC
    li, e_li = torch.zeros((), dtype=torch.float64), 0.0
    if itc == "logits":
        S = c.S.double()
        rl, e_rl = _lse(S, 1)
        cl, e_cl = (rl, e_rl) if variant == "col_lse_over_row" else _lse(S, 0)
        cl_r, e_cl_r = _lse(S, 0)
        dg = S.diagonal()
        term = (rl - dg) + (cl - dg)
        rterm = (rl - dg) + (cl_r - dg)
        e_term = e_rl + e_cl_r + U * (rl - dg).abs() + U * (cl_r - dg).abs() + U * rterm.abs()
        div = B if variant == "itc_over_B" else 2 * B
        li = (term * lv).sum() / div
        e_li = (e_term.sum() + gamma(_depth(B, 1)) * rterm.abs().sum()) / (2 * B)
        ap, aq = S - rl[:, None], S - cl[None, :]
        pp, qq = torch.exp(ap), torch.exp(aq)
        eye2 = 2 * torch.eye(B, dtype=torch.float64)
        dS = W_ITC * (pp + qq - eye2) / div
        rpp = UF + 2 * U * ap.abs() + e_rl[:, None]
        rqq = UF + 2 * U * (S - cl_r[None, :]).abs() + e_cl_r[None, :]
        qr = torch.exp(S - cl_r[None, :])
        ref["d_logits"] = dS
        b["d_logits"] = W_ITC / (2 * B) * (pp * rpp + qr * rqq + 2 * TINY + U * (pp + qr) + U * (pp + qr - eye2).abs()) + (U + UF) * W_ITC / (2 * B) * (pp + qr - eye2).abs()
    elif itc == "global":
        li = torch.tensor(ITC_GLOBAL, dtype=torch.float64)
    # ---- ITM
    lm, e_lm = torch.zeros((), dtype=torch.float64), 0.0
    if itm:
        tt = c.t.double()
        lab = (1 - c.lt) if variant == "itm_label_flipped" else c.lt
        ls2, e_ls2 = _lse(tt, 1)
        picked = tt.gather(1, lab[:, None]).squeeze(1)
        term = ls2 - picked
        e_term = e_ls2 + U * term.abs()
        lm = (term * lv).sum() / B
        e_lm = (e_term.sum() + gamma(_depth(B, 1)) * term.abs().sum()) / B
        dt = tt - ls2[:, None]
        pt = torch.exp(dt)
        rpt = UF + 2 * U * dt.abs() + e_ls2[:, None]
        oh = torch.zeros(B, 2, dtype=torch.float64).scatter_(1, lab[:, None], 1.0)
        ref["d_out_tim"] = W_ITM * (pt - oh) / B * lv[:, None]
        b["d_out_tim"] = W_ITM / B * (pt * rpt + TINY + U * (pt - oh).abs()) + (U + UF) * W_ITM / B * (pt - oh).abs()
    parts = (W_CLS * lc, W_ITC * li if itc != "off" else 0.0 * li, W_ITM * lm)
    ref["loss"] = torch.stack([parts[0] + parts[1] + parts[2], lc, li, lm])
    e_tot = W_CLS * e_lc + W_ITC * e_li + W_ITM * e_lm + (gamma(3) + U) * sum(x.abs() for x in parts)
    b["loss"] = torch.stack([torch.as_tensor(x, dtype=torch.float64) for x in (e_tot, e_lc + U * lc.abs(), e_li + U * li.abs() if itc == "logits" else 0.0,
                                                                                e_lm + U * lm.abs())])
    return ref, b


def corrupts(variant, c, class_w, itc, itm):
    """names of the outputs a wrong variant changes in this configuration (empty: it does not apply)"""
    if variant == "col_lse_over_row":
        return ("loss", "d_logits") if itc == "logits" and c.B > 1 else ()
    if variant == "no_wy":
        return ("d_out_cls",) if class_w or bool((c.y.sum(1) != 1).any()) else ()
    if variant == "itc_over_B":
        return ("loss", "d_logits") if itc == "logits" and c.B > 1 else ()          # B = 1: the term and its gradient are 0 over any divisor
    if variant == "itm_label_flipped":
        return ("loss", "d_out_tim") if itm else ()
    if variant == "rows_from_256_skipped":
        return (("loss", "d_out_cls") + (("d_out_tim",) if itm else ())) if c.B > 256 else ()
    raise ValueError(variant)


def emulate(c, class_w, itc, itm):
    """the same in fp32 (torch on the CPU: sums in another order than the kernel's, which the bounds allow for)"""
    f = torch.float32
    B, C = c.B, c.C
    z, y = c.z, c.y.to(f)
    w = (c.cw if class_w else torch.ones(C, dtype=f))[None, :]
    out = {}

    def lse32(x, dim):
        mx = x.max(dim=dim, keepdim=True).values
        return (mx + torch.log(torch.exp(x - mx).sum(dim=dim, keepdim=True))).squeeze(dim)

    lse = lse32(z, 1)
    lc = -((w * y * (z - lse[:, None])).sum()) / B
    wy = (w * y).sum(1, keepdim=True)
    out["d_out_cls"] = torch.tensor(W_CLS, dtype=f) * (torch.exp(z - lse[:, None]) * wy - w * y) / B
    li = torch.zeros((), dtype=f)
    if itc == "logits":
        S = c.S
        rl, cl = lse32(S, 1), lse32(S, 0)
        dg = S.diagonal()
        li = ((rl - dg) + (cl - dg)).sum() / (2.0 * B)
        out["d_logits"] = torch.tensor(W_ITC, dtype=f) * (torch.exp(S - rl[:, None]) + torch.exp(S - cl[None, :]) - 2 * torch.eye(B, dtype=f)) / (2.0 * B)
    elif itc == "global":
        li = torch.tensor(ITC_GLOBAL, dtype=f)
    lm = torch.zeros((), dtype=f)
    if itm:
        ls2 = lse32(c.t, 1)
        lm = (ls2 - c.t.gather(1, c.lt[:, None]).squeeze(1)).sum() / B
        oh = torch.zeros(B, 2, dtype=f).scatter_(1, c.lt[:, None], 1.0)
        out["d_out_tim"] = torch.tensor(W_ITM, dtype=f) * (torch.exp(c.t - ls2[:, None]) - oh) / B
    tot = torch.tensor(W_CLS, dtype=f) * lc + (torch.tensor(W_ITC, dtype=f) * li if itc != "off" else 0.0) + (torch.tensor(W_ITM, dtype=f) * lm if itm else 0.0)
    out["loss"] = torch.stack([tot, lc, li, lm])
    return out
