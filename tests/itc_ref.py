"""fp64 reference and per-element bounds of the rank-local ITC pair (include/mmhip.h mmhip_op_itc_fwd / mmhip_op_itc_bwd; csrc/heads.hip itc_norm_kernel,
itc_logits_kernel, itc_bwd_kernel), an fp32 emulation and two wrong variants (pure torch on the CPU: tests/test_itc_bounds_cpu.py checks the bounds,
tests/test_gpu_ops_itc.py the kernels).

    inv = 1 / |e|,  n = e inv,  S = exp(logit_scale) T_n I_n^T;      d n_t[i] = exp(logit_scale) sum_j dS_ij I_n[j]  (images: sum_i dS_ij T_n[i]),
    d e = (d n - n (d n . n)) inv,   d logit_scale += sum_ij dS_ij S_ij

Constants as in tests/test_gpu_ops_itc_global.py: u = U_32, uf = SLACK u for one __expf / square root / reciprocal, gamma(k) = k u / (1 - k u) for a sum of k
fp32 terms in any order.  First-order terms only.
  forward   s = sum e^2 (E products, E - 1 additions, all terms >= 0): relative gamma(E + 1);  inv: r = gamma(E + 1) / 2 + 2 uf;  n: |n| (r + u)
            es = __expf(logit_scale): relative re = uf + |logit_scale| u (the argument is scaled to base 2 first)
            S_ij: es ((r_t[i] + r_i[j] + 2 u + gamma(E)) A_ij + |c_ij| (re + u)),  A = |T_n| |I_n|^T, c = T_n I_n^T  (the kernel dots its own stored rows)
  backward  (fed the reference's rows, logits and 1 / |e| as fp32 -- the forward's rounding is not charged to it)
            d n[c] = es sum_j dl_j o_j[c]: B fused multiply-adds in sequence, one product: e_dn = es gamma(B) sum_j |dl_j o_j[c]| + |d n| (re + u)
            dot = sum_c d n[c] n[c]: e_dot = sum_c e_dn |n| + gamma(E + 1) sum_c |d n n|
            d e = (d n - n dot) inv: (e_dn + |n| e_dot + 2 u (|d n| + |n dot|)) inv + u |d e|
            d logit_scale: gamma(B^2 + 2) (|prefill| + sum |dl S|)   (B^2 products and additions, the add onto what the word holds)"""
import math
from types import SimpleNamespace

import torch

from op_bounds import SLACK, U_32

SHAPES = [(1, 4), (2, 1), (5, 255), (5, 257), (64, 512), (65, 1024)]          # (B, E)
LOGIT_SCALES = [0.0, math.log(1 / 0.07), math.log(100.0)]
U, UF = U_32, SLACK * U_32


def gamma(k):
    return k * U / (1.0 - k * U)


def make_inputs(B, E, ls, seed=0):
    """raw projections of very different row norms (matching pairs likeliest, as in training), a d_logits that is NOT symmetric, a prefill"""
    g = torch.Generator().manual_seed(77 * B + E + seed)
    t = torch.randn(B, E, generator=g)
    i = t + 0.7 * torch.randn(B, E, generator=g)
    t = t * (0.05 + 4 * torch.rand(B, 1, generator=g))
    i = i * (0.05 + 4 * torch.rand(B, 1, generator=g))
    dl = 0.1 * torch.randn(B, B, generator=g) + 0.05
    return SimpleNamespace(B=B, E=E, te=t.float().contiguous(), ie=i.float().contiguous(), ls=torch.tensor([ls], dtype=torch.float32),
                           dl=dl.float().contiguous(), pre_dls=3.0)


def fwd_reference(c):
    te, ie = c.te.double(), c.ie.double()
    es = math.exp(float(c.ls.double()))
    tinv, iinv = 1.0 / te.norm(dim=1), 1.0 / ie.norm(dim=1)
    tn, im = te * tinv[:, None], ie * iinv[:, None]
    cc = tn @ im.t()
    r = gamma(c.E + 1) / 2 + 2 * UF
    re = UF + abs(float(c.ls)) * U
    ref = dict(txt_inv=tinv, img_inv=iinv, txt_n=tn, img_n=im, logits=es * cc)
    b = dict(txt_inv=tinv * r, img_inv=iinv * r, txt_n=tn.abs() * (r + U), img_n=im.abs() * (r + U),
             logits=es * ((2 * r + 2 * U + gamma(c.E)) * (tn.abs() @ im.abs().t()) + cc.abs() * (re + U)))
    return ref, b


def logits_bound_given_rows(tn, im, ls):
    """bound of S against es tn im^T for rows taken AS GIVEN (the cross-check: both pairs dot the same stored rows)"""
    tn, im = tn.double(), im.double()
    es, re = math.exp(float(ls)), UF + abs(float(ls)) * U
    return es * (gamma(tn.shape[1]) * (tn.abs() @ im.abs().t()) + (tn @ im.t()).abs() * (re + U))


def bwd_inputs(c, fr):
    """what the backward kernel reads, as fp32: the reference's rows, 1 / |e| and logits"""
    f = lambda t: t.float().contiguous()
    return SimpleNamespace(tn=f(fr["txt_n"]), im=f(fr["img_n"]), tinv=f(fr["txt_inv"]), iinv=f(fr["img_inv"]), logits=f(fr["logits"]))


def bwd_reference(c, bi, dl=None, mutant=None, extra_dl_err=None):
    """fp64 on the fp32 inputs.  mutant: "swap" (rows and columns of d_logits swapped in the image gradient), "no_projection" (n (d n . n) left out).
    extra_dl_err: |error| of dl itself against the quantity the caller compares with (the cross-check), carried through both products."""
    dl = (c.dl if dl is None else dl).double()
    es, re = math.exp(float(c.ls.double())), UF + abs(float(c.ls)) * U
    B, E = c.B, c.E
    tn, im = bi.tn.double(), bi.im.double()
    ref, b = {}, {}
    for name, mine, other, w, inv in (("d_txt_e", tn, im, dl, bi.tinv.double()), ("d_img_e", im, tn, dl if mutant == "swap" else dl.t(), bi.iinv.double())):
        dn = es * (w @ other)
        e_dn = es * gamma(B) * (w.abs() @ other.abs()) + dn.abs() * (re + U)
        if extra_dl_err is not None:
            e_dn = e_dn + es * ((extra_dl_err if name == "d_txt_e" else extra_dl_err.t()) @ other.abs())
        dot = (dn * mine).sum(1, keepdim=True)
        e_dot = (e_dn * mine.abs()).sum(1, keepdim=True) + gamma(E + 1) * (dn * mine).abs().sum(1, keepdim=True)
        proj = 0.0 if mutant == "no_projection" else mine * dot
        ref[name] = (dn - proj) * inv[:, None]
        b[name] = (e_dn + mine.abs() * e_dot + 2 * U * (dn.abs() + (mine * dot).abs())) * inv[:, None] + U * ref[name].abs()
    terms = dl * bi.logits.double()
    ref["d_logit_scale"] = (c.pre_dls + terms.sum()).reshape(1)
    b["d_logit_scale"] = (gamma(B * B + 2) * (abs(c.pre_dls) + terms.abs().sum())).reshape(1)
    return ref, b


def emulate(c, bi):
    """both directions in fp32, in the kernels' order of operations"""
    f = torch.float32
    out = {}
    for name, e in (("txt", c.te), ("img", c.ie)):
        inv = 1.0 / torch.sqrt((e * e).sum(1))
        out[name + "_inv"], out[name + "_n"] = inv, e * inv[:, None]
    es = torch.exp(c.ls)[0]
    out["logits"] = (out["txt_n"] @ out["img_n"].t()) * es
    for name, mine, other, w, inv in (("d_txt_e", bi.tn, bi.im, c.dl, bi.tinv), ("d_img_e", bi.im, bi.tn, c.dl.t(), bi.iinv)):
        dn = (w @ other) * es
        dot = (dn * mine).sum(1, keepdim=True)
        out[name] = (dn - mine * dot) * inv[:, None]
    out["d_logit_scale"] = (torch.tensor(c.pre_dls, dtype=f) + (c.dl * bi.logits).sum()).reshape(1)
    return out


def global_reference(tn, im, ls, seed):
    """the global pair's outputs for G = B_local (rank offset 0) on the rows AS GIVEN, with the bounds derived in tests/test_gpu_ops_itc_global.py
    (the same closed forms, for arbitrary rows and logit_scale): logits S, dS, d T_n, d I_n and their bounds"""
    T, I = tn.double(), im.double()
    G, E = T.shape
    es = math.exp(float(ls))
    c = T @ I.t()
    S = es * c
    rl, cl = torch.logsumexp(S, dim=1), torch.logsumexp(S, dim=0)
    eye = torch.eye(G, dtype=torch.float64)
    p, q = torch.exp(S - rl[:, None]), torch.exp(S - cl[None, :])
    dS = seed / (2 * G) * (p + q - 2 * eye)
    u, uf, logG = U, UF, math.log(G)
    nt = (G + 31) // 32
    bS = es * (gamma(E) * (T.abs() @ I.abs().t()) + c.abs() * (uf + u))
    rho = 2 * (uf + 2 * es * u) + u + gamma(31) + gamma(nt)
    own = rho + uf * logG + u * (es + logG)
    b_rl, b_cl = bS.max(dim=1).values + own, bS.max(dim=0).values + own
    a = bS + b_rl[:, None] + u * (2 * es + logG) + uf
    b = bS + b_cl[None, :] + u * (2 * es + logG) + uf
    bgs = seed / (2 * G) * es * (p * a + q * b + (p + q + 2 * eye) * (4 * u + uf))
    gs = es * dS
    return SimpleNamespace(S=S, bS=bS, dS=dS, b_dS=bgs / es, dT=gs @ I, dI=gs.t() @ T, b_dT=bgs @ I.abs() + gamma(G) * (gs.abs() @ I.abs()),
                           b_dI=bgs.t() @ T.abs() + gamma(G) * (gs.t().abs() @ T.abs()))


def normalisation_bound(dn, e_dn, n, inv):
    """d e = (d n - n (d n . n)) inv from a d n known within e_dn: the propagated part and the arithmetic of tests/test_gpu_ops_itc_global.py's
    normalisation test (a dot of E fp32 products, then a product, a subtraction and a product)"""
    dn, n, inv = dn.double(), n.double(), inv.double()[:, None]
    E = n.shape[1]
    dot = (dn * n).sum(1, keepdim=True)
    prop = e_dn + n.abs() * (e_dn * n.abs()).sum(1, keepdim=True)
    arith = gamma(E) * (dn.abs() * n.abs()).sum(1, keepdim=True) * n.abs() + 3 * U * (dn.abs() + (n * dot).abs())
    return (prop + arith) * inv
