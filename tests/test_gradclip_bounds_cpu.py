"""CPU: the bounds tests/test_gpu_ops_gradclip.py holds the clipping kernels to (tests/gradclip_ref.py) admit an fp32 computation in the kernels' order
of summation and reject six wrong variants, for every case the GPU test runs; and the reference's coefficient is torch.nn.utils.clip_grad_norm_'s."""
import math

import numpy as np
import pytest
import torch

import gradclip_ref as GR

ALL = [(c, m) for c in GR.CASES for m in GR.MODES] + [("zeros", "zeros")]


@pytest.mark.parametrize("case,mode", ALL)
def test_emulation_inside_and_wrong_variants_outside(case, mode):
    inp = GR.build(case, mode)
    ref = GR.reference(inp)
    total, coef, clipped = GR.emulate(inp)
    print("margins", case, mode, "k", ref.k, "total", abs(total - ref.total) / ref.b_total if ref.b_total else 0.0,
          "coef", abs(coef - ref.coef) / ref.b_coef if ref.b_coef else 0.0)
    assert not GR.outside(inp, total, coef, ref), (total, ref.total, ref.b_total, coef, ref.coef, ref.b_coef)
    assert clipped == ref.clipped
    if mode == "half":
        assert 0.45 < ref.coef < 0.5001 and ref.clipped          # (the smallest cases have norms near 1e-3, where the epsilon is already felt)
    if mode == "eps":
        assert 0.5e-5 < ref.total < 2e-5 and abs(ref.coef - ref.total / (ref.total + 1e-6)) < 1e-5 and 0.8 < ref.coef < 0.96
    if mode in ("under", "zeros"):
        assert ref.coef == 1.0 and ref.b_coef == 0.0 and coef == 1.0
    if mode == "zeros":
        assert ref.total == 0.0 and total == 0.0
    tried = 0
    for v in GR.VARIANTS:
        if GR.applies(v, case, mode):
            w = GR.reference(inp, v)
            assert GR.outside(inp, w.total, w.coef, ref), (v, w.total, ref.total, ref.b_total, w.coef, ref.coef, ref.b_coef)
            tried += 1
    assert tried >= 1


def test_every_variant_is_tried_somewhere():
    for v in GR.VARIANTS:
        assert any(GR.applies(v, c, m) for c, m in ALL), v


def test_the_bound_follows_the_tree_depth():
    """k = serial fused multiply-adds + 10 + 1: one trip of the main loop is 4 per accumulator, the first element past a full trip starts the next"""
    k = lambda case: GR.reference(GR.build(case, "half")).k
    assert k("n4") == 4 + 11 and k("n7") == 5 + 11 and k("n3") == 1 + 11
    assert k("pass") == 4 + 11 and k("pass-4") == 4 + 11 and k("pass+7") == 9 + 11 and k("3pass+1027") == 17 + 11
    assert k("seg16") == sum(4 * (n >= 4) + (n % 4 != 0) for n in GR.SEG16) + 11
    assert k("rows7x8") == 4 * 4 + 11          # the four flagged rows of one chunk, one four-vector per lane and row


@pytest.mark.parametrize("max_norm", [0.05, 1.0, 1e9])
def test_reference_coefficient_is_torchs(max_norm):
    g = torch.Generator().manual_seed(3)
    params = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in ((5, 7), (13,), (1,), (3, 4, 5))]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).double()          # fp32 values: what the reference reads, held in fp64 so that torch adds no rounding of its own
    before = [p.grad.clone() for p in params]
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
    inp = GR.SimpleNamespace(segs=[b.flatten().numpy().astype(np.float32) for b in before], table=None, state=None, gs=1.0, max_norm=max_norm)
    ref = GR.reference(inp)
    assert math.isclose(float(norm), ref.total, rel_tol=1e-12)
    for p, b in zip(params, before):
        assert torch.allclose(p.grad, b * ref.coef, rtol=1e-12, atol=0.0)
    assert (ref.coef == 1.0) == (max_norm >= float(norm) + 1e-6)
