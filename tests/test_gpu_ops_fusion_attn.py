"""-m gpu: the CLS-query fusion attention (include/mmhip.h mmhip_op_fusion_attn_fwd / _bwd; csrc/heads.hip fusion_attn_fwd_kernel, fusion_attn_bwd_kernel)
against the fp64 reference and the derived per-element bounds of tests/fusion_attn_ref.py (tests/test_fusion_attn_bounds_cpu.py shows that an fp32
computation is inside them and four wrong variants are outside): every element of prob, xbar and dqk, outputs between sentinels.  The backward is
handed the reference's weights rounded to fp32, so the forward's rounding is not charged to it."""
import pytest
import torch

import fusion_attn_ref as FR
import gpu_util as gu

pytestmark = pytest.mark.gpu


def _guarded(shapes):
    return {n: gu.guarded(s, torch.float32, float("nan")) for n, s in shapes.items()}


def _intact(out, what):
    for n, (buf, view, snap) in out.items():
        assert gu.guards_intact(buf, snap, view.numel()), f"{what}: {n} written outside its buffer"


@pytest.mark.parametrize("dt", FR.DTYPES)
@pytest.mark.parametrize("P,H", FR.SHAPES)
def test_fusion_attn_against_float64(P, H, dt):
    dev, code = gu.dev(), gu.DT[dt][0]
    worst = {}
    for Bt, B in FR.BT_B:
        c = FR.make_inputs(dt, Bt, B, P, H)
        what = f"fusion attention {dt} Bt={Bt} B={B} P={P} H={H}"
        fr, fb = FR.fwd_reference(c)
        prob = fr["prob"].float()
        br, bb = FR.bwd_reference(c, prob)
        xv, qk, dxbar, probd = c.xv.to(dev), c.qk.to(dev), c.dxbar.to(dev), prob.to(dev)
        out = _guarded(dict(prob=(Bt, P), xbar=(Bt, H)))
        gu.call("mmhip_op_fusion_attn_fwd", code, gu.ptr(qk), gu.ptr(xv), Bt, B, P, H, c.scale, gu.ptr(out["prob"][1]), gu.ptr(out["xbar"][1]), gu.stream())
        bout = _guarded(dict(dqk=(Bt, H)))
        gu.call("mmhip_op_fusion_attn_bwd", code, gu.ptr(dxbar), gu.ptr(probd), gu.ptr(xv), Bt, B, P, H, c.scale, gu.ptr(bout["dqk"][1]), gu.stream())
        torch.cuda.synchronize()
        _intact(out, what)
        _intact(bout, what)
        for n in fr:
            worst[n] = max(worst.get(n, 0.0), gu.assert_close_elementwise(out[n][1], fr[n], fb[n], f"{what}: {n}"))
        worst["dqk"] = max(worst.get("dqk", 0.0), gu.assert_close_elementwise(bout["dqk"][1], br["dqk"], bb["dqk"], f"{what}: dqk"))
    print("margins fusion_attn", (P, H, dt), {k: round(x, 4) for k, x in worst.items()})


@pytest.mark.parametrize("kw", [dict(P=513), dict(H=1028), dict(H=770), dict(B=0)], ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_fusion_attn_rejects_on_the_host(kw):
    """MMHIP_E_INVALID from both entry points before anything is launched: the outputs keep their sentinel bytes"""
    dev, lib = gu.dev(), gu._lib.lib()
    p = dict(Bt=2, B=2, P=4, H=8)
    p.update(kw)
    x = torch.zeros(2 * 4 * 8, dtype=torch.bfloat16, device=dev)
    rows = torch.zeros(2, 8, device=dev)
    outs = [torch.full(s, 7.0, device=dev) for s in ((2, 4), (2, 8), (2, 8))]
    prob, xbar, dqk = outs
    for code in (gu._lib.BF16, gu._lib.F16, gu._lib.F32):
        assert lib.mmhip_op_fusion_attn_fwd(code, gu.ptr(rows), gu.ptr(x), p["Bt"], p["B"], p["P"], p["H"], 1.0, gu.ptr(prob), gu.ptr(xbar), gu.stream()) == -1
        assert lib.mmhip_op_fusion_attn_bwd(code, gu.ptr(rows), gu.ptr(prob), gu.ptr(x), p["Bt"], p["B"], p["P"], p["H"], 1.0, gu.ptr(dqk), gu.stream()) == -1
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs)
