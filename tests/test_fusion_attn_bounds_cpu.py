"""No GPU: the bounds of tests/fusion_attn_ref.py hold for an fp32 computation on every case tests/test_gpu_ops_fusion_attn.py runs, and four wrong
variants leave them wherever they compute something else: the tokens of post bt instead of bt % B, the last token dropped, the scale missing in the
backward, the sum_i p_i dp_i term missing."""
import pytest
import torch

import fusion_attn_ref as FR
from gpu_util import assert_close_elementwise, violates_elementwise


@pytest.mark.parametrize("dt", FR.DTYPES)
@pytest.mark.parametrize("P,H", FR.SHAPES)
def test_fp32_computation_stays_inside_and_wrong_variants_leave(P, H, dt):
    for Bt, B in FR.BT_B:
        c = FR.make_inputs(dt, Bt, B, P, H)
        what = f"{dt} Bt={Bt} B={B} P={P} H={H}"
        fr, fb = FR.fwd_reference(c)
        prob = fr["prob"].float()
        br, bb = FR.bwd_reference(c, prob)
        emu = FR.emulate(c, prob)
        for ref, bound in ((fr, fb), (br, bb)):
            for name in ref:
                assert assert_close_elementwise(emu[name], ref[name], bound[name], f"emulated {name} {what}") <= 1
        s = c.scale * torch.einsum("bh,bph->bp", c.qk.double(), c.xv.double()[torch.arange(Bt) % B])
        assert P < 31 or s.abs().max() > 20, what          # the spread the max subtraction is there for
        assert P < 2 or 0.5 < fr["prob"][0, -1] < 0.99, what      # row 0: the last token dominates, the others still count
        assert Bt < 3 or P < 2 or fr["prob"][2].max() > 0.999, what      # row 2: one token all but alone
        for variant in FR.VARIANTS:
            if not FR.applies(variant, c):
                continue
            if variant in ("tokens_of_post_bt", "last_token_dropped"):
                wrong = FR.fwd_reference(c, variant=variant)
                for name in ("prob", "xbar") if P > 1 else ("xbar",):          # (P = 1: the one weight is 1 whichever token it is)
                    assert violates_elementwise(wrong[name], fr[name], fb[name]) > 0, (variant, name, what)
            if variant != "last_token_dropped" and P > 1:          # (P = 1: the backward's result is 0 whatever the tokens)
                wrong = FR.bwd_reference(c, prob, variant=variant)
                assert violates_elementwise(wrong["dqk"], br["dqk"], bb["dqk"]) > 0, (variant, what)


def test_entry_points_reject_on_the_host():
    """MMHIP_E_INVALID without touching a pointer or launching anything"""
    import ctypes as C
    from smtc_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()
    one, odd = C.c_void_p(256), C.c_void_p(264)

    def both(dtype=_lib.BF16, rows=one, xv=one, Bt=2, B=2, P=4, H=8, o1=one, o2=one):
        return (lib.mmhip_op_fusion_attn_fwd(dtype, rows, xv, Bt, B, P, H, 1.0, o1, o2, None),
                lib.mmhip_op_fusion_attn_bwd(dtype, rows, o1, xv, Bt, B, P, H, 1.0, o2, None))

    for kw in (dict(P=513), dict(H=1028), dict(H=770), dict(H=0), dict(B=0), dict(Bt=0), dict(P=0), dict(dtype=_lib.PAIR), dict(dtype=-1), dict(rows=None),
               dict(xv=None), dict(o1=None), dict(o2=None), dict(rows=odd), dict(xv=odd)):
        assert both(**kw) == (-1, -1), kw
