"""-m gpu: the global-batch ITC operator pair (include/mmhip.h mmhip_op_itc_global_fwd / _bwd; csrc/heads.hip) against a float64 torch computation of

    S = exp(logit_scale) T_n I_n^T  [G, G],   loss = (CE(S, arange) + CE(S^T, arange)) / 2        (reference models/utils.py:225-231 clip_loss)
    dS = seed / (2 G) (softmax_rows(S) + softmax_cols(S) - 2 I),   d T_n[i] = exp(logit_scale) sum_j dS_ij I_n[j],   d I_n[j] = exp(logit_scale) sum_i dS_ij T_n[i]
    d logit_scale = sum_{i local, j} dS_ij S_ij                                                   (the local text rows' strip)

per element, every bound derived below from the kernels' rounding points.  Constants: u = U_32 = 2^-24; uf = SLACK * u for one expf / logf result
(op_bounds.SLACK: about an ulp each); gamma(n) = n u / (1 - n u), the error factor of a sum of n fp32 terms in any order.  First-order terms only.

  es      = expf(logit_scale):                      relative uf
  S_ij    = fl(es * dot_E(T_n[i], I_n[j])):         dS_ij  = es (gamma(E) A_ij + |c_ij| (uf + u)),  A = |T_n| |I_n|^T, c = T_n I_n^T
            (the dot is an fmaf chain over E products split over 8 waves whose partials are added: E - 1 additions in some order)
  lse     log-sum-exp is 1-Lipschitz in the max norm, so the errors of S move it by at most max_j dS_ij.  Its own arithmetic: every
            expf(S - m) has relative error uf + u |S - m| <= uf + 2 es u (rounded argument); 32 of them are added per tile (gamma(31)); the G / 32
            tile sums are rescaled by expf(m_t - M) (again uf + 2 es u, and u for the product) and added (gamma(nt)); logf turns the relative
            error rho = 2 (uf + 2 es u) + u + gamma(31) + gamma(nt) of the sum into an absolute one and adds uf |log s| <= uf log G; the
            final M + log s rounds once: u (es + log G).     d_lse_i = max_j dS_ij + rho + uf log G + u (es + log G)
  loss    term_i = (rowlse_i - S_ii) + (collse_i - S_ii): t_i = d_rowlse_i + d_collse_i + 2 dS_ii + 3 u (2 es + log G) (three roundings of values
            below 2 es + log G each); sum of G terms in a fixed order, one division:  (sum t_i + gamma(G) sum |term_i|) / (2 G) + u |loss|
  dS es   p = expf(S - rowlse_i) has relative error a_ij = dS_ij + d_rowlse_i + u (2 es + log G) + uf, q = expf(S - collse_j) likewise with
            d_collse_j (b_ij); two additions, the products by seed / (2 G) and by es (its own uf):
            dgs_ij = seed / (2 G) es (p a_ij + q b_ij + (p + q + 2 [i = j]) (4 u + uf))
  d T_n   a [Bl, G] x [G, E] fp32 product of the stored dS es strip:  sum_j dgs_ij |I_n[j][c]| + gamma(G) sum_j |dS_ij es| |I_n[j][c]|;  d I_n alike
  d logit_scale  terms dS_ij S_ij: error dgs_ij / es |S_ij| + |dS_ij| dS_ij + u |dS_ij S_ij| each; they are added two per thread, over a wave (6
            steps), over 8 waves, the tile partials 'ceil(n / 256)' per thread, over a wave, over 4 waves, and into the output: a tree of depth
            D = 2 + 6 + 8 + ceil(n_tiles / 256) + 6 + 4 + 1:  gamma(D) sum |dS_ij S_ij|
"""
import math

import pytest
import torch

import gpu_util as gu
from op_bounds import SLACK, U_32

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 1, 8), (33, 11, 22, 64), (256, 64, 128, 512), (520, 65, 0, 512)]        # (G, B_local, rank_offset, E)
LOGIT_SCALE = 2.6592          # the dual encoder's initial value (exp = 14.3)
SEED = 1.75                   # seed of the backward: world * w_itc in the engine; any float here


def gamma(n):
    return n * U_32 / (1.0 - n * U_32)


_CASES = {}


def case(G, Bl, r0, E):
    """inputs (fp32, as the kernels get them), the float64 reference and the bounds of one shape: computed once, shared, never modified"""
    key = (G, Bl, r0, E)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(1000 + G)
    t = torch.randn(G, E, generator=g)
    i = t + 0.7 * torch.randn(G, E, generator=g)          # matching pairs are the likeliest: the diagonal dominates, as in training
    tn = (t / t.norm(dim=1, keepdim=True)).float().contiguous()
    im = (i / i.norm(dim=1, keepdim=True)).float().contiguous()
    ls = torch.tensor([LOGIT_SCALE], dtype=torch.float32)
    T, I = tn.double(), im.double()
    es = math.exp(float(ls.double()))
    c = T @ I.t()
    S = es * c
    rl, cl = torch.logsumexp(S, dim=1), torch.logsumexp(S, dim=0)
    d = S.diagonal()
    term = (rl - d) + (cl - d)
    loss = term.sum() / (2 * G)
    eye = torch.eye(G, dtype=torch.float64)
    p, q = torch.exp(S - rl[:, None]), torch.exp(S - cl[None, :])
    dS = SEED / (2 * G) * (p + q - 2 * eye)
    loc = slice(r0, r0 + Bl)
    dT = es * dS[loc, :] @ I
    dI = es * dS[:, loc].t() @ T
    dls = (dS[loc, :] * S[loc, :]).sum()
    # ---- bounds
    u, uf, logG = U_32, SLACK * U_32, math.log(G)
    nt = (G + 31) // 32
    bS = es * (gamma(E) * (T.abs() @ I.abs().t()) + c.abs() * (uf + u))
    rho = 2 * (uf + 2 * es * u) + u + gamma(31) + gamma(nt)
    own = rho + uf * logG + u * (es + logG)
    b_rl, b_cl = bS.max(dim=1).values + own, bS.max(dim=0).values + own
    t_i = b_rl + b_cl + 2 * bS.diagonal() + 3 * u * (2 * es + logG)
    b_loss = (t_i.sum() + gamma(G) * term.abs().sum()) / (2 * G) + u * loss.abs()
    a = bS + b_rl[:, None] + u * (2 * es + logG) + uf
    b = bS + b_cl[None, :] + u * (2 * es + logG) + uf
    bgs = SEED / (2 * G) * es * (p * a + q * b + (p + q + 2 * eye) * (4 * u + uf))
    gs = es * dS
    b_dT = bgs[loc, :] @ I.abs() + gamma(G) * (gs[loc, :].abs() @ I.abs())
    b_dI = bgs[:, loc].t() @ T.abs() + gamma(G) * (gs[:, loc].t().abs() @ T.abs())
    n_tiles = ((Bl + 31) // 32) * nt
    D = 2 + 6 + 8 + (n_tiles + 255) // 256 + 6 + 4 + 1
    prod = dS[loc, :] * S[loc, :]
    b_dls = (bgs[loc, :] / es * S[loc, :].abs() + dS[loc, :].abs() * bS[loc, :] + u * prod.abs()).sum() + gamma(D) * prod.abs().sum()
    r = dict(tn=tn, im=im, ls=ls, S=S, rl=rl, cl=cl, loss=loss.reshape(1), dT=dT, dI=dI, dls=dls.reshape(1), bS=bS, b_rl=b_rl, b_cl=b_cl,
             b_loss=b_loss.reshape(1), b_dT=b_dT, b_dI=b_dI, b_dls=b_dls.reshape(1))
    _CASES[key] = r
    return r


def run_pair(r, G, Bl, r0, E, want_logits=True):
    """forward + backward on the device; outputs sit between sentinels"""
    dev = gu.dev()
    tn, im, ls = r["tn"].to(dev), r["im"].to(dev), r["ls"].to(dev)
    nbytes = gu._lib.lib().mmhip_op_itc_global_ws_bytes(G, Bl)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = {}
    for name, shape in (("logits", (G, G)), ("rl", (G,)), ("cl", (G,)), ("loss", (1,)), ("dT", (Bl, E)), ("dI", (Bl, E)), ("dls", (1,))):
        out[name] = gu.guarded(shape, torch.float32, 0.0 if name == "dls" else float("nan"))
    v = lambda n: out[n][1]
    gu.call("mmhip_op_itc_global_fwd", gu.ptr(tn), gu.ptr(im), gu.ptr(ls), G, E, gu.ptr(v("logits")) if want_logits else None, gu.ptr(v("rl")),
            gu.ptr(v("cl")), gu.ptr(v("loss")), gu.ptr(ws), nbytes, gu.stream())
    gu.call("mmhip_op_itc_global_bwd", gu.ptr(tn), gu.ptr(im), gu.ptr(ls), gu.ptr(v("rl")), gu.ptr(v("cl")), G, Bl, r0, E, SEED, gu.ptr(v("dT")),
            gu.ptr(v("dI")), gu.ptr(v("dls")), None, None, None, None, gu.ptr(ws), nbytes, gu.stream())
    torch.cuda.synchronize()
    for name, (buf, view, snap) in out.items():
        assert gu.guards_intact(buf, snap, view.numel()), f"{name}: written outside its buffer"
    return {k: v(k).clone() for k in out}


@pytest.mark.parametrize("G,Bl,r0,E", SHAPES)
def test_itc_global_against_float64(G, Bl, r0, E):
    r = case(G, Bl, r0, E)
    got = run_pair(r, G, Bl, r0, E)
    margins = {}
    for name, ref, bound in (("logits", "S", "bS"), ("rl", "rl", "b_rl"), ("cl", "cl", "b_cl"), ("loss", "loss", "b_loss"), ("dT", "dT", "b_dT"),
                             ("dI", "dI", "b_dI"), ("dls", "dls", "b_dls")):
        margins[name] = gu.assert_close_elementwise(got[name], r[ref], r[bound], f"itc_global {name} G={G} Bl={Bl} r0={r0} E={E}")
    print("margins", (G, Bl, r0, E), {k: round(v, 4) for k, v in margins.items()})


@pytest.mark.parametrize("G,Bl,r0,E", SHAPES)
def test_itc_global_same_bits_twice(G, Bl, r0, E, monkeypatch):
    monkeypatch.setenv("MMHIP_DETERMINISTIC", "1")
    r = case(G, Bl, r0, E)
    a, b = run_pair(r, G, Bl, r0, E), run_pair(r, G, Bl, r0, E, want_logits=False)
    for k in a:
        if k != "logits":
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_itc_global_normalisation_backward_and_accumulation():
    """d e = (d n - n (d n . n)) / |e| of the local rows, from the d n the same call returns (the rule of launch_itc_bwd); d logit_scale is added to"""
    G, Bl, r0, E = 33, 11, 22, 64
    r = case(G, Bl, r0, E)
    dev = gu.dev()
    tn, im, ls = r["tn"].to(dev), r["im"].to(dev), r["ls"].to(dev)
    nbytes = gu._lib.lib().mmhip_op_itc_global_ws_bytes(G, Bl)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rl, cl, loss = torch.empty(G, device=dev), torch.empty(G, device=dev), torch.empty(1, device=dev)
    gu.call("mmhip_op_itc_global_fwd", gu.ptr(tn), gu.ptr(im), gu.ptr(ls), G, E, None, gu.ptr(rl), gu.ptr(cl), gu.ptr(loss), gu.ptr(ws), nbytes, gu.stream())
    inv_t, inv_i = torch.rand(Bl, device=dev) + 0.5, torch.rand(Bl, device=dev) + 0.5
    dT, dI, dte, die = (torch.empty(Bl, E, device=dev) for _ in range(4))
    dls = torch.full((1,), 3.0, device=dev)
    gu.call("mmhip_op_itc_global_bwd", gu.ptr(tn), gu.ptr(im), gu.ptr(ls), gu.ptr(rl), gu.ptr(cl), G, Bl, r0, E, SEED, gu.ptr(dT), gu.ptr(dI), gu.ptr(dls),
            gu.ptr(inv_t), gu.ptr(inv_i), gu.ptr(dte), gu.ptr(die), gu.ptr(ws), nbytes, gu.stream())
    torch.cuda.synchronize()
    for dn, n, inv, de in ((dT, tn[r0:r0 + Bl], inv_t, dte), (dI, im[r0:r0 + Bl], inv_i, die)):
        dn, n, inv = dn.double().cpu(), n.double().cpu(), inv.double().cpu()
        dot = (dn * n).sum(dim=1, keepdim=True)
        ref = (dn - n * dot) * inv[:, None]
        # the dot of E fp32 products (gamma(E) on sum |dn n|), then a product, a subtraction and a product: three roundings of values below |dn| + |n dot|
        bound = (gamma(E) * (dn.abs() * n.abs()).sum(dim=1, keepdim=True) * n.abs() + 3 * U_32 * (dn.abs() + (n * dot).abs())) * inv[:, None]
        gu.assert_close_elementwise(de, ref, bound, "itc_global d e")
    gu.assert_close_elementwise(dls, r["dls"] + 3.0, r["b_dls"] + U_32 * (r["dls"].abs() + 3.0), "itc_global d logit_scale accumulated")


@pytest.mark.parametrize("G,Bl,r0,E", [(8193, 4, 0, 8), (4, 2, 0, 1025), (16, 8, 9, 8)])
def test_itc_global_rejects_on_the_host(G, Bl, r0, E):
    """G > 8192, E > 1024, rank_offset + B_local > G: MMHIP_E_INVALID before anything is launched -- the outputs keep their bytes.  (The buffers have
    the sizes the call names.)"""
    dev = gu.dev()
    lib = gu._lib.lib()
    tn = torch.zeros(G, E, device=dev)
    ls = torch.zeros(1, device=dev)
    nbytes = (4 * ((G + 31) // 32) + 2) * G * 4 + 2 * Bl * G * 4 + 4096
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rl, cl, loss, dls = (torch.full((n,), 7.0, device=dev) for n in (G, G, 1, 1))
    dT, dI = torch.full((Bl, E), 7.0, device=dev), torch.full((Bl, E), 7.0, device=dev)
    if r0 + Bl <= G:          # a shape the forward must refuse
        assert lib.mmhip_op_itc_global_ws_bytes(G, Bl) == 0 or E > 1024
        rc = lib.mmhip_op_itc_global_fwd(gu.ptr(tn), gu.ptr(tn), gu.ptr(ls), G, E, None, gu.ptr(rl), gu.ptr(cl), gu.ptr(loss), gu.ptr(ws), nbytes, gu.stream())
        assert rc == -1, rc
    rc = lib.mmhip_op_itc_global_bwd(gu.ptr(tn), gu.ptr(tn), gu.ptr(ls), gu.ptr(rl), gu.ptr(cl), G, Bl, r0, E, 1.0, gu.ptr(dT), gu.ptr(dI), gu.ptr(dls), None, None,
                                     None, None, gu.ptr(ws), nbytes, gu.stream())
    assert rc == -1, rc
    torch.cuda.synchronize()
    for t in (rl, cl, loss, dls, dT, dI):
        assert bool((t == 7.0).all())
