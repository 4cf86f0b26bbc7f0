"""-m gpu: the heads' fp32 GEMM and bias gradient (include/mmhip.h mmhip_op_small_gemm / mmhip_op_bias_grad_f32; csrc/gemm.hip small_gemm_kernel behind
launch_small_nt / _nn / _tn, csrc/heads.hip bias_grad_f32_kernel) against the fp64 reference and the derived per-element bounds of
tests/small_gemm_ref.py (tests/test_small_gemm_bounds_cpu.py shows that an fp32 computation is inside them and four wrong variants are outside):
every element of the output, the output between sentinels, the columns between its rows bit-identical, NaN between the operands' rows."""
import pytest
import torch

import gpu_util as gu
import small_gemm_ref as SG

pytestmark = pytest.mark.gpu

CASES = SG.cases()
CODES = {"f32": gu._lib.F32, "bf16": gu._lib.BF16, "f16": gu._lib.F16}


def _dev(flat, off):
    """the flat buffer on the device and the pointer `off` elements in"""
    t = flat.to(gu.dev())
    return t, gu.C.c_void_p(t.data_ptr() + off * t.element_size())


@pytest.mark.parametrize("cs", CASES, ids=lambda c: c.id)
def test_small_gemm_against_float64(cs):
    r = SG.make_inputs(cs)
    ref, bound = SG.reference(r)
    a_t, a_p = _dev(r.A_flat, r.a_off)
    w_t, w_p = (a_t, gu.C.c_void_p(a_t.data_ptr() + 4 * r.w_off)) if cs.window else _dev(r.W_flat, r.w_off)
    bias = r.bias.to(gu.dev()) if cs.bias else None
    buf, out, snap = gu.guarded((cs.M, r.ldo), torch.float32, 0.0)
    out.copy_(r.out0)
    gu.call("mmhip_op_small_gemm", cs.mode, CODES[cs.a_dtype], a_p, r.lda, w_p, r.ldw, gu.ptr(bias), gu.ptr(out), r.ldo, cs.M, cs.N, cs.K, cs.act, cs.acc,
            gu.stream())
    torch.cuda.synchronize()
    assert gu.guards_intact(buf, snap, out.numel()), f"{cs.id}: written outside out"
    got = out.cpu()
    assert torch.equal(got[:, cs.N:].view(torch.int32), r.out0[:, cs.N:].view(torch.int32)), f"{cs.id}: written between the rows of out"
    m = gu.assert_close_elementwise(got[:, :cs.N], ref, bound, f"small gemm {cs.id}")
    print("margins small_gemm", cs.id, round(m, 4))


@pytest.mark.parametrize("cols", SG.BG_COLS)
@pytest.mark.parametrize("rows", SG.BG_ROWS)
def test_bias_grad_f32_against_float64(rows, cols):
    r = SG.bias_grad_inputs(rows, cols)
    d = r.d_flat.to(gu.dev())
    worst = 0.0
    for acc in (0, 1):
        ref, bound = SG.bias_grad_reference(r, acc)
        buf, out, snap = gu.guarded((cols,), torch.float32, 0.0)
        out.copy_(r.out0)
        gu.call("mmhip_op_bias_grad_f32", gu.ptr(d), rows, cols, r.ld, gu.ptr(out), acc, gu.stream())
        torch.cuda.synchronize()
        assert gu.guards_intact(buf, snap, cols), f"bias gradient {rows}x{cols}: written outside out"
        worst = max(worst, gu.assert_close_elementwise(out, ref, bound, f"bias gradient {rows}x{cols} acc={acc}"))
    print("margins bias_grad_f32", (rows, cols), round(worst, 4))


@pytest.mark.parametrize("kw", [dict(M=0), dict(K=0), dict(mode=3), dict(act=3), dict(lda=7), dict(ldw=7), dict(ldo=7), dict(mode=1, a_dtype="bf16")],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_small_gemm_rejects_on_the_host(kw):
    """MMHIP_E_INVALID before the launch: the output keeps its bytes"""
    dev, lib = gu.dev(), gu._lib.lib()
    A, W, out = torch.zeros(8, 8, device=dev), torch.zeros(8, 8, device=dev), torch.full((8, 8), 7.0, device=dev)
    p = dict(mode=0, a_dtype="f32", lda=8, ldw=8, ldo=8, M=8, N=8, K=8, act=0)
    p.update(kw)
    assert lib.mmhip_op_small_gemm(p["mode"], CODES[p["a_dtype"]], gu.ptr(A), p["lda"], gu.ptr(W), p["ldw"], None, gu.ptr(out), p["ldo"], p["M"], p["N"], p["K"],
                                   p["act"], 0, gu.stream()) == -1
    assert lib.mmhip_op_bias_grad_f32(gu.ptr(A), 8, 8, 7, gu.ptr(out), 0, gu.stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
