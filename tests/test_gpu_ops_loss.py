"""-m gpu: the fused loss mix (include/mmhip.h mmhip_op_loss; csrc/heads.hip loss_kernel) against the fp64 reference and the derived per-element bounds
of tests/loss_ref.py (tests/test_loss_bounds_cpu.py shows that an fp32 computation is inside them and five wrong variants are outside): loss[0..3] and
every element of the three gradients, outputs between sentinels, n_correct held to equality; with every optional output NULL the loss is the same bits."""
import itertools

import pytest
import torch

import gpu_util as gu
import loss_ref as LR

pytestmark = pytest.mark.gpu

CONFIGS = list(itertools.product((False, True), LR.ITC_MODES, (False, True)))
_CASES = {}


def case(B, C):
    """inputs on the host and the device: made once, shared, never modified"""
    if (B, C) not in _CASES:
        c = LR.make_inputs(B, C)
        d = {k: getattr(c, k).to(gu.dev()).contiguous() for k in ("z", "y", "cw", "S", "t", "lt")}
        d["glob"] = torch.tensor([LR.ITC_GLOBAL], device=gu.dev())
        _CASES[(B, C)] = (c, d, LR.n_correct(c))
    return _CASES[(B, C)]


def run(c, d, class_w, itc, itm, outputs=True):
    B, C = c.B, c.C
    out = {"loss": gu.guarded((4,), torch.float32, float("nan")), "d_out_cls": gu.guarded((B, C), torch.float32, float("nan")),
           "d_logits": gu.guarded((B, B), torch.float32, float("nan")), "d_out_tim": gu.guarded((B, 2), torch.float32, float("nan")),
           "n_correct": gu.guarded((1,), torch.int32, -7)}
    v = lambda n: gu.ptr(out[n][1]) if outputs else None
    gu.call("mmhip_op_loss", gu.ptr(d["z"]), gu.ptr(d["y"]), gu.ptr(d["cw"]) if class_w else None, gu.ptr(d["S"]) if itc == "logits" else None,
            gu.ptr(d["glob"]) if itc == "global" else None, gu.ptr(d["t"]) if itm else None, gu.ptr(d["lt"]) if itm else None, LR.W_CLS, LR.W_ITC, LR.W_ITM,
            B, C, gu.ptr(out["loss"][1]), v("d_out_cls"), v("d_logits"), v("d_out_tim"), v("n_correct"), gu.stream())
    torch.cuda.synchronize()
    for n, (buf, view, snap) in out.items():
        assert gu.guards_intact(buf, snap, view.numel()), f"{n}: written outside its buffer"
    return {n: o[1].clone() for n, o in out.items()}


@pytest.mark.parametrize("B,C", LR.BC)
def test_loss_against_float64(B, C):
    c, d, correct = case(B, C)
    worst = {}
    for class_w, itc, itm in CONFIGS:
        what = f"loss B={B} C={C} class_w={class_w} itc={itc} itm={itm}"
        ref, bound = LR.reference(c, class_w, itc, itm)
        got = run(c, d, class_w, itc, itm)
        for n in ref:
            worst[n] = max(worst.get(n, 0.0), gu.assert_close_elementwise(got[n], ref[n], bound[n], f"{what}: {n}"))
        assert int(got["n_correct"].item()) == correct, what
        # a gradient whose term is off is not written
        for n in ("d_logits", "d_out_tim"):
            assert n in ref or bool(torch.isnan(got[n]).all()), f"{what}: {n} written"
        # every optional output NULL: the same loss bits, nothing else written
        bare = run(c, d, class_w, itc, itm, outputs=False)
        assert torch.equal(bare["loss"], got["loss"]), what
        assert all(bool(torch.isnan(bare[n]).all()) for n in ("d_out_cls", "d_logits", "d_out_tim")) and int(bare["n_correct"].item()) == -7, what
    print("margins loss", (B, C), {k: round(x, 4) for k, x in worst.items()})


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=1025), dict(C=0), dict(tim_without_labels=True), dict(both_itc=True), dict(no_loss=True)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_loss_rejects_on_the_host(kw):
    """MMHIP_E_INVALID before the launch: the outputs keep their bytes"""
    dev, lib = gu.dev(), gu._lib.lib()
    B, C = kw.get("B", 4), kw.get("C", 3)
    z, y = torch.zeros(4, 3, device=dev), torch.zeros(4, 3, dtype=torch.int64, device=dev)
    S, t, lt, one = torch.zeros(4, 4, device=dev), torch.zeros(4, 2, device=dev), torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(1, device=dev)
    outs = [torch.full(s, 7.0, device=dev) for s in ((4,), (4, 3), (4, 4), (4, 2))]
    nc = torch.full((1,), 7, dtype=torch.int32, device=dev)
    rc = lib.mmhip_op_loss(gu.ptr(z), gu.ptr(y), None, gu.ptr(S) if kw.get("both_itc") else None, gu.ptr(one) if kw.get("both_itc") else None,
                           gu.ptr(t) if kw.get("tim_without_labels") else None, None, 1.0, 0.1, 0.1, B, C, None if kw.get("no_loss") else gu.ptr(outs[0]),
                           gu.ptr(outs[1]), gu.ptr(outs[2]), gu.ptr(outs[3]), gu.ptr(nc), gu.stream())
    assert rc == -1
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs) and int(nc.item()) == 7
