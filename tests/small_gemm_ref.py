"""fp64 reference and per-element bounds of the heads' fp32 GEMM and bias gradient (include/mmhip.h mmhip_op_small_gemm / mmhip_op_bias_grad_f32;
csrc/gemm.hip small_gemm_kernel behind launch_small_nt / _nn / _tn, csrc/heads.hip bias_grad_f32_kernel), an fp32 emulation and four wrong
variants (pure torch on the CPU: tests/test_small_gemm_bounds_cpu.py checks the bounds, tests/test_gpu_ops_small_gemm.py the kernels).

    out[M, N] (+)= act(P + bias);   NT: P = A[M, K] W[N, K]^T,   NN: P = A[M, K] W[K, N],   TN: P = A[K, M]^T W[K, N]

Operands are laid out as the kernel meets them: a flat buffer, the matrix `off` elements in, rows `ld` apart; what lies between the rows is NaN (a
read outside a row poisons the result), what lies between the rows of `out` must keep its bytes.
Constants: u = U_32, gamma(k) = k u / (1 - k u).  Terms, summed and times SLACK:
    P       a workgroup's 8 waves take 8-wide slices of K in turn: a wave chains 8 ceil(K / 64) fused multiply-adds (never more than K), the 8 partial
            tiles are added in sequence: gamma(min(K, 8 ceil(K / 64)) + 8) |A| |B|        (a 16-bit A is exact in fp32)
    bias    u |P + bias|
    tanh    (1 - t^2) e_pre + 4 u |t|      (tanhf: 2 ulp);      relu: e_pre (|relu x - relu y| <= |x - y|)
    accumulate   u |out0 + v|
    bias gradient  out0 + sum_r d[r]: gamma(rows + 1) (|out0| + sum_r |d|)"""
from types import SimpleNamespace

import torch

from op_bounds import SLACK, U_32

U = U_32
NT, NN, TN = 0, 1, 2
MODE_NAMES = {NT: "nt", NN: "nn", TN: "tn"}
MN = [1, 2, 3, 31, 32, 33, 65, 128]
KS = [1, 3, 4, 5, 8, 61, 64, 67, 768, 1536]
VARIANTS = ("k_tail_dropped", "other_modes_strides", "accumulate_ignored", "act_before_bias")
BG_ROWS, BG_COLS = [1, 5, 128], [1, 3, 255, 256, 257, 768]


def gamma(k):
    return k * U / (1.0 - k * U)


def _case(mode, M, N, K, c, a_dtype="f32", window=False):
    """flags from the running counter c: leading dimensions padded by one, bases offset by one element, bias, activation, accumulate"""
    return SimpleNamespace(mode=mode, M=M, N=N, K=K, a_dtype=a_dtype, ld_pad=c & 1, off_a=(c >> 1) & 1, off_w=(c >> 2) & 1, bias=c % 3 != 0, act=c % 3,
                           acc=int(c % 4 == 1), window=window, id=f"{MODE_NAMES[mode]}-{a_dtype}-{M}x{N}x{K}-c{c}" + ("-win" if window else ""))


def cases():
    out = []
    for mode in (NT, NN, TN):
        c = mode
        for i, K in enumerate(KS):
            for j in range(3):
                out.append(_case(mode, MN[(3 * i + 5 * j + mode) % 8], MN[(i + 3 * j + 2 * mode + 1) % 8], K, c))
                c += 1
        out.append(_case(mode, 128, 768, 1536, 5))          # the largest: bias, relu, accumulate, padded, base of A offset
    for n, (K, dt) in enumerate([(3, "bf16"), (64, "f16"), (67, "bf16"), (67, "f16"), (768, "bf16"), (8, "f16"), (5, "bf16"), (1536, "f16")]):
        out.append(_case(NT, MN[(2 * n + 3) % 8], MN[(3 * n + 1) % 8], K, (1, 5, 7, 10, 13, 17, 11, 21)[n], a_dtype=dt))
    # TN on column windows of one wider matrix (the engine's z + H, ld = ZW), two output columns (the ITM head), reduction over the posts
    for n, (K, M) in enumerate([(3, 32), (64, 33), (67, 128), (128, 65), (5, 1), (61, 768)]):
        out.append(_case(TN, M, 2, K, 2 * n, window=True))
    return out


def storage(rows, cols, ld, off, values):
    """flat fp32 buffer holding `values` [rows, cols] `off` elements in with rows `ld` apart, NaN elsewhere"""
    flat = torch.full((off + rows * ld,), float("nan"), dtype=values.dtype)
    flat[off:].view(rows, ld)[:, :cols] = values
    return flat


def make_inputs(cs):
    g = torch.Generator().manual_seed(cs.M * 131 + cs.N * 17 + cs.K + cs.mode)
    M, N, K = cs.M, cs.N, cs.K
    a_shape = (K, M) if cs.mode == TN else (M, K)
    w_shape = (N, K) if cs.mode == NT else (K, N)
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[cs.a_dtype]
    A = torch.randn(a_shape, generator=g).to(tdt)
    # tanh cases: products of order 1 and a small bias, so that the activation is not saturated (a saturated tanh hides its argument)
    W = (torch.randn(w_shape, generator=g) * (K ** -0.5 if cs.act == 1 else 1.0)).float()
    r = SimpleNamespace(cs=cs, A=A, W=W)
    if cs.window:          # both operands are column windows of one [K, ZW] matrix: A at column H, W at column H + M
        H = 4 + cs.off_a
        ZW = H + M + N + 3
        z = torch.randn(K, ZW, generator=g).float()
        r.A, r.W = z[:, H:H + M].clone(), z[:, H + M:H + M + N].clone()
        r.A_flat = r.W_flat = z.reshape(-1).clone()
        r.lda = r.ldw = ZW
        r.a_off, r.w_off = H, H + M
    else:
        r.lda, r.ldw = a_shape[1] + cs.ld_pad, w_shape[1] + cs.ld_pad
        r.a_off, r.w_off = cs.off_a, cs.off_w
        r.A_flat = storage(a_shape[0], a_shape[1], r.lda, r.a_off, A)
        r.W_flat = storage(w_shape[0], w_shape[1], r.ldw, r.w_off, W)
    r.ldo = N + cs.ld_pad
    r.bias = (torch.randn(N, generator=g) * (0.3 if cs.act == 1 else 1.0)).float() if cs.bias else None
    r.out0 = torch.randn(M, r.ldo, generator=g).float()          # what `out` holds before the call, the columns past N included
    return r


def _read(flat, off, s_outer, s_inner, n_outer, n_inner):
    """[n_outer, n_inner] matrix read from flat storage with the given element strides; what lies past the buffer reads as 0"""
    idx = off + torch.arange(n_outer)[:, None] * s_outer + torch.arange(n_inner)[None, :] * s_inner
    pad = torch.cat([flat.double(), torch.zeros(max(0, int(idx.max()) + 1 - flat.numel()), dtype=torch.float64)])
    return pad[idx]


def reference(r, variant=None):
    """fp64 out[:, :N] and its bound.  variant: one of VARIANTS (the bound stays that of the right formula)"""
    cs = r.cs
    M, N, K = cs.M, cs.N, cs.K
    A = (r.A.double().t() if cs.mode == TN else r.A.double())          # [M, K]
    B = (r.W.double().t() if cs.mode == NT else r.W.double())          # [K, N]
    Bv, Kv = B, K
    if variant == "other_modes_strides":          # NT's W read as [K, N] rows ldw apart, NN / TN's as [N, K]
        Bv = _read(r.W_flat, r.w_off, r.ldw, 1, K, N) if cs.mode == NT else _read(r.W_flat, r.w_off, 1, r.ldw, K, N)
        Bv = torch.nan_to_num(Bv, nan=0.0)
    if variant == "k_tail_dropped":
        Kv = K - (K & 3)
    P = A[:, :Kv] @ Bv[:Kv]
    bias = r.bias.double()[None, :] if cs.bias else 0.0
    act = {0: lambda x: x, 1: torch.tanh, 2: lambda x: x.clamp_min(0.0)}[cs.act]
    v = act(P) + bias if variant == "act_before_bias" else act(P + bias)
    out0 = r.out0.double()[:, :N]
    res = v + out0 if (cs.acc and variant != "accumulate_ignored") else v
    if variant is not None:
        return res
    e = gamma(min(K, 8 * ((K + 63) // 64)) + 8) * (A.abs() @ B.abs())
    if cs.bias:
        e = e + U * (P + bias).abs()
    if cs.act == 1:
        e = (1.0 - v * v) * e + 4 * U * v.abs()
    if cs.acc:
        e = e + U * res.abs()
    return res, SLACK * e


def applies(variant, r):
    """whether a wrong variant computes something else on this case (the two stride orders meet the same elements when ldw = 1 or W is 1 x 1)"""
    cs = r.cs
    return {"k_tail_dropped": cs.K & 3 != 0, "other_modes_strides": (cs.K > 1 or cs.N > 1) and r.ldw != 1, "accumulate_ignored": bool(cs.acc),
            "act_before_bias": bool(cs.act and cs.bias)}[variant]


def emulate(r):
    """fp32: one product in torch's order, then the epilogue as the kernel applies it"""
    cs = r.cs
    A = r.A.float().t() if cs.mode == TN else r.A.float()
    B = r.W.t() if cs.mode == NT else r.W
    v = A @ B
    if cs.bias:
        v = v + r.bias[None, :]
    v = torch.tanh(v) if cs.act == 1 else (v.clamp_min(0.0) if cs.act == 2 else v)
    return r.out0[:, :cs.N] + v if cs.acc else v


def bias_grad_inputs(rows, cols):
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    ld = cols + 3
    d = torch.randn(rows, cols, generator=g).float() + 0.25
    return SimpleNamespace(rows=rows, cols=cols, ld=ld, d=d, d_flat=storage(rows, cols, ld, 0, d), out0=torch.randn(cols, generator=g).float())


def bias_grad_reference(r, acc, variant=None):
    s = r.d.double().sum(0)
    res = s + r.out0.double() if (acc and variant != "accumulate_ignored") else s
    if variant is not None:
        return res
    return res, SLACK * gamma(r.rows + 1) * ((r.out0.double().abs() if acc else 0.0) + r.d.double().abs().sum(0))
