"""No GPU: the bounds of tests/itc_ref.py (the rank-local ITC pair) hold for an fp32 computation in the kernels' order on every case
tests/test_gpu_ops_itc.py runs, and two wrong backward variants leave them: rows and columns of d_logits swapped in the image gradient, and the
projection term n (d n . n) of the normalisation backward left out."""
import pytest
import torch

import itc_ref as IR
from gpu_util import assert_close_elementwise, violates_elementwise


@pytest.mark.parametrize("ls", IR.LOGIT_SCALES, ids=lambda v: f"ls{v:.2f}")
@pytest.mark.parametrize("B,E", IR.SHAPES)
def test_fp32_computation_stays_inside(B, E, ls):
    c = IR.make_inputs(B, E, ls)
    fr, fb = IR.fwd_reference(c)
    bi = IR.bwd_inputs(c, fr)
    br, bb = IR.bwd_reference(c, bi)
    emu = IR.emulate(c, bi)
    for ref, bound in ((fr, fb), (br, bb)):
        for name in ref:
            assert assert_close_elementwise(emu[name], ref[name], bound[name], f"emulated {name}") <= 1


@pytest.mark.parametrize("ls", IR.LOGIT_SCALES, ids=lambda v: f"ls{v:.2f}")
@pytest.mark.parametrize("B,E", [s for s in IR.SHAPES if s[0] > 1])
def test_wrong_backward_variants_leave_the_bounds(B, E, ls):
    c = IR.make_inputs(B, E, ls)
    assert not torch.equal(c.dl, c.dl.t())
    fr, _ = IR.fwd_reference(c)
    bi = IR.bwd_inputs(c, fr)
    br, bb = IR.bwd_reference(c, bi)
    swapped, _ = IR.bwd_reference(c, bi, mutant="swap")
    if E > 1:          # E = 1: d e = (d n - n (d n n)) / |e| is 0 whatever d_logits holds (n = +-1): no function of d_logits can be seen in it
        assert violates_elementwise(swapped["d_img_e"], br["d_img_e"], bb["d_img_e"]) > 0
    else:
        assert (br["d_img_e"] == 0).all() and (swapped["d_img_e"] == 0).all()
    flat, _ = IR.bwd_reference(c, bi, mutant="no_projection")
    for name in ("d_txt_e", "d_img_e"):          # (E = 1: the reference is exactly 0 -- a unit scalar has no tangent -- and the variant is d n / |e|)
        assert violates_elementwise(flat[name], br[name], bb[name]) > 0, name


def test_entry_points_reject_on_the_host():
    """E > 1024 and B < 1: MMHIP_E_INVALID without touching a pointer or launching anything"""
    import ctypes as C
    from smtc_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()
    one = C.c_void_p(256)
    for B, E in ((4, 1025), (0, 8), (-1, 8)):
        assert lib.mmhip_op_itc_fwd(one, one, one, B, E, one, one, one, one, one, None) == -1
        assert lib.mmhip_op_itc_bwd(one, one, one, one, one, one, one, B, E, one, one, one, None) == -1
