"""No GPU: the bounds of tests/small_gemm_ref.py hold for an fp32 computation on every case tests/test_gpu_ops_small_gemm.py runs, and four wrong
variants leave them wherever they compute something else: the K & 3 tail dropped, W read with the other mode's strides, accumulate ignored, the
activation applied before the bias.  Also: the case list reaches every size and flag the kernel branches on."""
import pytest

import small_gemm_ref as SG
from gpu_util import assert_close_elementwise, violates_elementwise

CASES = SG.cases()


def test_case_list_reaches_every_edge():
    for mode in (SG.NT, SG.NN, SG.TN):
        cs = [c for c in CASES if c.mode == mode and not c.window]
        assert {c.K for c in cs} >= set(SG.KS) and {c.M for c in cs} >= set(SG.MN) and {c.N for c in cs} >= set(SG.MN), mode
        for flag in ("ld_pad", "off_a", "off_w", "acc"):
            assert {getattr(c, flag) for c in cs} == {0, 1}, (mode, flag)
        assert {c.act for c in cs} == {0, 1, 2} and {c.bias for c in cs} == {False, True}
        assert 24 <= len(cs) <= 48
    assert {c.a_dtype for c in CASES if c.mode == SG.NT} == {"f32", "bf16", "f16"} and all(c.a_dtype == "f32" for c in CASES if c.mode != SG.NT)
    assert any(c.window and c.N == 2 for c in CASES) and max(c.M * c.N * c.K for c in CASES) == 128 * 768 * 1536
    assert len({c.id for c in CASES}) == len(CASES)


@pytest.mark.parametrize("cs", CASES, ids=lambda c: c.id)
def test_fp32_computation_stays_inside_and_wrong_variants_leave(cs):
    r = SG.make_inputs(cs)
    ref, bound = SG.reference(r)
    assert assert_close_elementwise(SG.emulate(r), ref, bound, f"emulated {cs.id}") <= 1
    for variant in SG.VARIANTS:
        if SG.applies(variant, r):
            assert violates_elementwise(SG.reference(r, variant=variant), ref, bound) > 0, (variant, cs.id)


def test_every_variant_is_seen_in_every_mode_and_dtype():
    for key in {(c.mode, c.a_dtype) for c in CASES}:
        rs = [SG.make_inputs(c) for c in CASES if (c.mode, c.a_dtype) == key and c.M * c.N * c.K < 1 << 20]
        for variant in SG.VARIANTS:
            assert any(SG.applies(variant, r) for r in rs), (key, variant)


@pytest.mark.parametrize("cols", SG.BG_COLS)
@pytest.mark.parametrize("rows", SG.BG_ROWS)
def test_bias_gradient_bounds(rows, cols):
    r = SG.bias_grad_inputs(rows, cols)
    for acc in (0, 1):
        ref, bound = SG.bias_grad_reference(r, acc)
        emu = r.d.sum(0) + (r.out0 if acc else 0.0)
        assert assert_close_elementwise(emu, ref, bound, f"emulated bias gradient {rows}x{cols} acc={acc}") <= 1
    ref, bound = SG.bias_grad_reference(r, 1)
    assert violates_elementwise(SG.bias_grad_reference(r, 1, variant="accumulate_ignored"), ref, bound) > 0


def test_entry_points_reject_on_the_host():
    """MMHIP_E_INVALID without touching a pointer or launching anything"""
    import ctypes as C
    from smtc_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()
    one = C.c_void_p(256)

    def gemm(mode=0, a_dtype=_lib.F32, A=one, lda=8, W=one, ldw=8, out=one, ldo=8, M=8, N=8, K=8, act=0):
        return lib.mmhip_op_small_gemm(mode, a_dtype, A, lda, W, ldw, None, out, ldo, M, N, K, act, 0, None)

    bad = [dict(A=None), dict(W=None), dict(out=None), dict(M=0), dict(N=0), dict(K=0), dict(K=-1), dict(mode=3), dict(mode=-1), dict(act=3), dict(act=-1),
           dict(a_dtype=_lib.PAIR), dict(mode=1, a_dtype=_lib.BF16), dict(mode=2, a_dtype=_lib.F16), dict(ldo=7), dict(lda=7), dict(ldw=7),
           dict(mode=1, lda=7), dict(mode=1, ldw=7, K=4), dict(mode=2, lda=7, K=4), dict(mode=2, ldw=7, K=4)]
    for kw in bad:
        assert gemm(**kw) == -1, kw
    for args in ((None, 4, 4, 4, one), (one, 4, 4, 4, None), (one, 0, 4, 4, one), (one, 4, 0, 4, one), (one, 4, 4, 3, one)):
        d, rows, cols, ld, out = args
        assert lib.mmhip_op_bias_grad_f32(d, rows, cols, ld, out, 0, None) == -1, args
