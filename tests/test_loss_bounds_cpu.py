"""No GPU: the bounds of tests/loss_ref.py (the fused loss mix) hold for an fp32 computation on every case tests/test_gpu_ops_loss.py runs, and five
wrong variants leave them in every output they corrupt: the column log-sum-exp taken over the row, the wy factor missing from d_out_cls, ITC divided
by B, the ITM label flipped, rows from 256 on skipped.  Also: what the inputs promise (gaps, planted ties, soft-target rows, an asymmetric S)."""
import itertools

import pytest
import torch

import loss_ref as LR
from gpu_util import assert_close_elementwise, violates_elementwise

CONFIGS = list(itertools.product((False, True), LR.ITC_MODES, (False, True)))
_CASES = {}


def case(B, C):
    if (B, C) not in _CASES:
        _CASES[(B, C)] = LR.make_inputs(B, C)
    return _CASES[(B, C)]


@pytest.mark.parametrize("B,C", LR.BC)
def test_inputs_are_what_the_cases_need(B, C):
    c = case(B, C)
    z = c.z.double()
    top2 = z.topk(2, dim=1).values
    gap = top2[:, 0] - top2[:, 1]
    tie = torch.zeros(B, dtype=torch.bool)
    tie[c.ties] = True
    assert bool((gap[~tie] >= LR.MIN_GAP).all()) and bool((gap[tie] == 0).all())
    assert c.ties == [r for r in LR.TIE_ROWS if r < B]
    for r in c.ties:
        assert LR.first_argmax(z)[r] == 0 and z[r, C - 1] == z[r, 0]
    assert z.abs().max() <= 80.5 and (B < 255 or z.abs().max() > 60)
    assert c.S.abs().max() <= 100 and (B < 3 or not torch.equal(c.S, c.S.t())) and (B < 255 or c.S.abs().max() == 100)
    if B >= 5:
        sums = c.y.sum(1)
        assert bool((sums == 0).any()) and bool((c.y == 2).any()) and bool(((sums == 2) & (c.y.max(1).values == 1)).any())
    if B >= 4:
        dom = c.S.diagonal() >= c.S.max(dim=1).values
        assert bool(dom.any()) and not bool(dom.all())
    assert 0 <= LR.n_correct(c) <= B


@pytest.mark.parametrize("B,C", LR.BC)
def test_fp32_computation_stays_inside(B, C):
    c = case(B, C)
    for class_w, itc, itm in CONFIGS:
        ref, bound = LR.reference(c, class_w, itc, itm)
        emu = LR.emulate(c, class_w, itc, itm)
        assert set(ref) == set(emu) == set(bound)
        for name in ref:
            assert assert_close_elementwise(emu[name], ref[name], bound[name], f"emulated {name} B={B} C={C} {class_w} {itc} {itm}") <= 1


@pytest.mark.parametrize("B,C", LR.BC)
def test_wrong_variants_leave_the_bounds(B, C):
    c = case(B, C)
    seen = set()
    for class_w, itc, itm in CONFIGS:
        ref, bound = LR.reference(c, class_w, itc, itm)
        for variant in LR.VARIANTS:
            names = LR.corrupts(variant, c, class_w, itc, itm)
            if not names:
                continue
            seen.add(variant)
            wrong, _ = LR.reference(c, class_w, itc, itm, variant=variant)
            for name in names:
                assert violates_elementwise(wrong[name], ref[name], bound[name]) > 0, (variant, name, B, C, class_w, itc, itm)
    assert {"itm_label_flipped", "no_wy"} <= seen and (B == 1 or {"itc_over_B", "col_lse_over_row"} <= seen) and (B <= 256 or "rows_from_256_skipped" in seen)


def test_entry_point_rejects_on_the_host():
    """MMHIP_E_INVALID without touching a pointer or launching anything"""
    import ctypes as C
    from smtc_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()
    one = C.c_void_p(256)

    def call(out_cls=one, onehot=one, lpt=None, glob=None, out_tim=None, lbl=None, B=4, Cc=3, loss=one):
        return lib.mmhip_op_loss(out_cls, onehot, None, lpt, glob, out_tim, lbl, 1.0, 0.1, 0.1, B, Cc, loss, None, None, None, None, None)

    for kw in (dict(out_cls=None), dict(onehot=None), dict(loss=None), dict(B=0), dict(B=-3), dict(B=1025), dict(Cc=0), dict(out_tim=one),
               dict(lpt=one, glob=one)):
        assert call(**kw) == -1, kw
