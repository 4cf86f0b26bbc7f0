"""-m gpu: the rank-local ITC operator pair (include/mmhip.h mmhip_op_itc_fwd / mmhip_op_itc_bwd; csrc/heads.hip itc_norm_kernel, itc_logits_kernel,
itc_bwd_kernel -- what both engines run unless --itc_global is on) against the fp64 reference and the derived per-element bounds of tests/itc_ref.py
(tests/test_itc_bounds_cpu.py shows that an fp32 computation is inside them and two wrong backwards are outside), every element of every output,
outputs between sentinels; and against the global pair at G = B_local = B, within the sum of the two pairs' bounds."""
import pytest
import torch

import gpu_util as gu
import itc_ref as IR

pytestmark = pytest.mark.gpu

_CASES = {}


def case(B, E, ls):
    """inputs, references and bounds of one case: computed once, shared, never modified"""
    key = (B, E, ls)
    if key not in _CASES:
        c = IR.make_inputs(B, E, ls)
        fr, fb = IR.fwd_reference(c)
        bi = IR.bwd_inputs(c, fr)
        br, bb = IR.bwd_reference(c, bi)
        _CASES[key] = (c, fr, fb, bi, br, bb)
    return _CASES[key]


FWD_OUT = (("txt_n", "BE"), ("img_n", "BE"), ("txt_inv", "B"), ("img_inv", "B"), ("logits", "BB"))


def run_fwd(c):
    dev = gu.dev()
    shp = {"BE": (c.B, c.E), "B": (c.B,), "BB": (c.B, c.B)}
    out = {n: gu.guarded(shp[s], torch.float32, float("nan")) for n, s in FWD_OUT}
    v = lambda n: out[n][1]
    te, ie, ls = c.te.to(dev), c.ie.to(dev), c.ls.to(dev)
    gu.call("mmhip_op_itc_fwd", gu.ptr(te), gu.ptr(ie), gu.ptr(ls), c.B, c.E, gu.ptr(v("txt_n")), gu.ptr(v("img_n")), gu.ptr(v("txt_inv")), gu.ptr(v("img_inv")),
            gu.ptr(v("logits")), gu.stream())
    torch.cuda.synchronize()
    for n, (buf, view, snap) in out.items():
        assert gu.guards_intact(buf, snap, view.numel()), f"{n}: written outside its buffer"
    return {n: v(n).clone() for n in out}


def run_bwd(c, dl, logits, tn, im, tinv, iinv, with_dls=True):
    dev = gu.dev()
    out = {"d_txt_e": gu.guarded((c.B, c.E), torch.float32, float("nan")), "d_img_e": gu.guarded((c.B, c.E), torch.float32, float("nan")),
           "d_logit_scale": gu.guarded((1,), torch.float32, c.pre_dls)}
    v = lambda n: out[n][1]
    ins = [t.to(dev).contiguous() for t in (dl, logits, tn, im, tinv, iinv, c.ls)]
    gu.call("mmhip_op_itc_bwd", *[gu.ptr(t) for t in ins], c.B, c.E, gu.ptr(v("d_txt_e")), gu.ptr(v("d_img_e")),
            gu.ptr(v("d_logit_scale")) if with_dls else None, gu.stream())
    torch.cuda.synchronize()
    for n, (buf, view, snap) in out.items():
        assert gu.guards_intact(buf, snap, view.numel()), f"{n}: written outside its buffer"
    return {n: v(n).clone() for n in out}


@pytest.mark.parametrize("ls", IR.LOGIT_SCALES, ids=lambda v: f"ls{v:.2f}")
@pytest.mark.parametrize("B,E", IR.SHAPES)
def test_itc_local_against_float64(B, E, ls):
    c, fr, fb, bi, br, bb = case(B, E, ls)
    got = run_fwd(c)
    margins = {n: gu.assert_close_elementwise(got[n], fr[n], fb[n], f"itc {n} B={B} E={E} ls={ls:.3f}") for n, _ in FWD_OUT}
    gb = run_bwd(c, c.dl, bi.logits, bi.tn, bi.im, bi.tinv, bi.iinv)
    for n in br:
        margins[n] = gu.assert_close_elementwise(gb[n], br[n], bb[n], f"itc {n} B={B} E={E} ls={ls:.3f}")
    print("margins itc", (B, E, round(ls, 3)), {k: round(v, 4) for k, v in margins.items()})
    # d_logit_scale null: the embedding gradients are the same bits, the word keeps its prefill
    g0 = run_bwd(c, c.dl, bi.logits, bi.tn, bi.im, bi.tinv, bi.iinv, with_dls=False)
    assert torch.equal(g0["d_txt_e"], gb["d_txt_e"]) and torch.equal(g0["d_img_e"], gb["d_img_e"]) and g0["d_logit_scale"].item() == c.pre_dls


@pytest.mark.parametrize("ls", IR.LOGIT_SCALES, ids=lambda v: f"ls{v:.2f}")
@pytest.mark.parametrize("B,E", IR.SHAPES)
def test_itc_local_agrees_with_the_global_pair(B, E, ls):
    """G = B_local = B: both pairs dot the rows the local forward stored, so the logits agree within the sum of the two products' bounds; the global
    backward forms dS itself, the local one is handed the fp64 dS of the same rows rounded to fp32 -- the embedding gradients agree within the local
    bound (the rounding of dS carried through) plus the global pair's d n bound carried through the normalisation backward."""
    c = case(B, E, ls)[0]
    seed = 1.75
    dev = gu.dev()
    lf = run_fwd(c)
    tn, im = lf["txt_n"].cpu(), lf["img_n"].cpu()
    nbytes = gu._lib.lib().mmhip_op_itc_global_ws_bytes(B, B)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    lg = torch.full((B, B), float("nan"), device=dev)
    rl, cl, loss = torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(1, device=dev)
    lsd = c.ls.to(dev)
    gu.call("mmhip_op_itc_global_fwd", gu.ptr(lf["txt_n"]), gu.ptr(lf["img_n"]), gu.ptr(lsd), B, E, gu.ptr(lg), gu.ptr(rl), gu.ptr(cl), gu.ptr(loss), gu.ptr(ws),
            nbytes, gu.stream())
    dT, dI, dte, die = (torch.full((B, E), float("nan"), device=dev) for _ in range(4))
    gu.call("mmhip_op_itc_global_bwd", gu.ptr(lf["txt_n"]), gu.ptr(lf["img_n"]), gu.ptr(lsd), gu.ptr(rl), gu.ptr(cl), B, B, 0, E, seed, gu.ptr(dT), gu.ptr(dI),
            None, gu.ptr(lf["txt_inv"]), gu.ptr(lf["img_inv"]), gu.ptr(dte), gu.ptr(die), gu.ptr(ws), nbytes, gu.stream())
    torch.cuda.synchronize()
    gr = IR.global_reference(tn, im, c.ls, seed)
    m = {"logits": gu.assert_close_elementwise(lf["logits"], lg.double().cpu(), IR.logits_bound_given_rows(tn, im, c.ls) + gr.bS, f"local vs global logits B={B} E={E}")}
    dl = gr.dS.float()
    bi = IR.bwd_inputs(c, dict(txt_n=tn, img_n=im, txt_inv=lf["txt_inv"].cpu(), img_inv=lf["img_inv"].cpu(), logits=lf["logits"].cpu()))
    _, lb = IR.bwd_reference(c, bi, dl=dl, extra_dl_err=(dl.double() - gr.dS).abs())
    loc = run_bwd(c, dl, bi.logits, bi.tn, bi.im, bi.tinv, bi.iinv)
    for name, got_g, dn, e_dn, n, inv in (("d_txt_e", dte, gr.dT, gr.b_dT, tn, bi.tinv), ("d_img_e", die, gr.dI, gr.b_dI, im, bi.iinv)):
        bound = lb[name] + IR.normalisation_bound(dn, e_dn, n, inv)
        m[name] = gu.assert_close_elementwise(loc[name], got_g.double().cpu(), bound, f"local vs global {name} B={B} E={E}")
    print("margins itc-vs-global", (B, E, round(ls, 3)), {k: round(v, 4) for k, v in m.items()})


@pytest.mark.parametrize("B,E", [(4, 1025), (0, 8), (-1, 8)])
def test_itc_local_rejects_on_the_host(B, E):
    """E > 1024 and B < 1: MMHIP_E_INVALID from both entry points before anything is launched -- the outputs keep their bytes"""
    dev = gu.dev()
    lib = gu._lib.lib()
    Bb = max(B, 1)
    x = torch.zeros(Bb, E, device=dev)
    sq, ls = torch.zeros(Bb, Bb, device=dev), torch.zeros(1, device=dev)
    outs = [torch.full(s, 7.0, device=dev) for s in ((Bb, E), (Bb, E), (Bb,), (Bb,), (Bb, Bb), (1,))]
    n1, n2, i1, i2, lgt, dls = outs
    assert lib.mmhip_op_itc_fwd(gu.ptr(x), gu.ptr(x), gu.ptr(ls), B, E, gu.ptr(n1), gu.ptr(n2), gu.ptr(i1), gu.ptr(i2), gu.ptr(lgt), gu.stream()) == -1
    assert lib.mmhip_op_itc_bwd(gu.ptr(sq), gu.ptr(sq), gu.ptr(x), gu.ptr(x), gu.ptr(i1), gu.ptr(i2), gu.ptr(ls), B, E, gu.ptr(n1), gu.ptr(n2), gu.ptr(dls),
                                gu.stream()) == -1
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == 7.0).all())
