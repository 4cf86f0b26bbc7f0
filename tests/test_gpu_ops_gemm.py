"""-m gpu: the GEMMs (mmhip_op_gemm_nt, mmhip_op_gemm_tn, mmhip_op_gemm_tn_group), LayerNorm forward / backward and mmhip_op_colsum per element against
fp64 with the derived bounds of tests/op_bounds.py (gemm_nt_reference, gemm_tn_reference, ln_bounds, ln_bwd_reference, colsum_reference), and -- through
mmhip_op_last_gemm_path -- the proof of WHICH kernel ran: the launchers fall back silently (a forced tile whose width does not divide N, a deep-pipelined
tile whose shape rules fail, unaligned operands, TN variant 4 with Nn % 256), so every case named after a kernel asserts that kernel.

Every (dtype, shape, slow) case of tests/test_gpu_ops.py's test_gemm_nt_epilogues / test_x3_gemm_nt / test_gemm_tn / test_x3_gemm_tn /
test_gemm_tn_group_matches_single_problems / test_layernorm_fwd_bwd / test_colsum_and_casts runs here as well (those tests keep their aggregate
assertions where they are); the per-element checks, NaN pre-fill, guard bands and path assertions are what this module adds.

Path coverage (each in bf16 and f16 unless noted; `slow` = tile code << 4, bit 0 = generic):
    NT tile kernels (gemm.hip)         1 128x128, 6 128x192, 9 role-specialised 256x128, 10 128x96, 12 role-specialised 256x96, 21 128x128 on a
                                       3-deep ring: the test_gpu_ops.py shapes + test_gemm_nt_tile_edges (K = 1, 2, ring depth, ring depth + 1
                                       k-tiles of 64; M = 1, BM - 1, BM + 1; N = 1 and 9 tiles wide; guard bands on every buffer)
    NT deep-pipelined (gemm8.hip)      13 / 15 256x256, 14 / 16 256x128, 17 / 18 256x192 (one-shot / persistent): the same two tests; the persistent
                                       loop with more tiles than workgroups on the 8192 / 12608 / 16384 / 35000 / 40000 / 70000-row shapes (asserted)
    NT default dispatch                (4096, 768, 2304) and (512, 768, 3072) -> 21; (300, 480, 128) -> 10; (12608, 2304, 768) -> 15, persistent, several
                                       tiles per workgroup; (12608, 768, 768) -> 17
    NT split-K                         test_gemm_nt_splitk (and not taken with tanh)
    NT generic                         slow = 1, and test_gemm_nt_unaligned_falls_back (A, B, C or the bias off 16-byte alignment)
    parity (x3, fp32 tensors)          direct, small, scratch-split and generic NT: test_x3_gemm_nt_per_element; TN direct and scratch-split
    TN variants 1 and 4, TN generic    test_gemm_tn_variants (Nn % 256 == 0 and == 128: 4 falls back to 1), test_gemm_tn_per_element, test_gemm_tn_edges
    TN group                           the test_gpu_ops.py group and one of more than mmhip_tn_max_group() fast problems (flush in the middle)

References: fp64 on the CPU; for shapes of more than 2048 rows the SAME op_bounds code runs on device tensors (torch's fp64 matmul and element-wise
kernels, none of them this project's), which keeps the module's wall time near that of the kernels it checks.  Margins are printed (pytest -s:
`MARGIN family ...`) and tabulated in profiles/op_test_margins.md."""
import ctypes as C

import pytest
import torch

import op_bounds as OB

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs an MI355X")]

if torch.cuda.is_available():
    from gpu_util import DT, dev, ptr, stream, call, assert_close_elementwise, guarded, guards_intact, keep_mask
    from smtc_amd import _lib

SEED, SID = 0x123456789ABCDEF, 21
VARIANTS = ("plain", "bias_gelu_aux", "bias_drop_resid", "mulgrad_resid", "bias_tanh_f32", "plain_f32")
TILE_FAMILY = {1: 2, 6: 2, 9: 2, 10: 2, 12: 2, 21: 2, 13: 3, 14: 3, 15: 3, 16: 3, 17: 3, 18: 3}      # _lib.NT_TILE / NT_DEEP
TILE_BM = {1: 128, 6: 128, 9: 256, 10: 128, 12: 256, 21: 128, 13: 256, 14: 256, 15: 256, 16: 256, 17: 256, 18: 256}
TILE_BN = {1: 128, 6: 192, 9: 128, 10: 96, 12: 96, 21: 128, 13: 256, 14: 128, 15: 256, 16: 128, 17: 192, 18: 192}
TILE_DEPTH = {1: 2, 6: 2, 9: 3, 10: 2, 12: 3, 21: 3, 13: 2, 14: 3, 15: 2, 16: 3, 17: 2, 18: 2}          # LDS ring depth in k-tiles of 64 (NTCfg NS, P8::NBUF)
# default dispatch the launcher documents (gemm.hip choose_nt_tile): (family, tile, persistent loop ran several tiles per workgroup or None = not asserted)
DEFAULT_PATH = {(4096, 768, 2304): (2, 21, None), (512, 768, 3072): (2, 21, None), (300, 480, 128): (2, 10, None),
                (12608, 2304, 768): (3, 15, 1), (12608, 768, 768): (3, 17, 0)}


def _check(got, ref, bound, what):
    """assert_close_elementwise, on the device when the reference lives there (the failure message comes from the CPU version)"""
    if ref.is_cuda:
        g = got.detach().double().reshape(ref.shape)
        err = (g - ref).abs()
        err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        worst = ratio.max().item()
        if worst <= 1.0:
            return worst
        ref, bound = ref.cpu(), bound.cpu()
    return assert_close_elementwise(got, ref, bound, what)


def _where(M, N=0):
    """where a case's fp64 reference is computed: on the device above 2048 rows (and for the many small edge cases, above 200 000 output elements)"""
    return dev() if (M > 2048 or M * N > 200000) else torch.device("cpu")


class _Buf:
    """a device tensor of `shape` holding `data` (or `fill`), inside guard bands when asked to"""

    def __init__(self, shape, tdt, data=None, fill=float("nan"), guard=False):
        self.n = 1
        for s in shape:
            self.n *= s
        if guard:
            self.buf, self.t, self.snap = guarded(shape, tdt, fill)
        else:
            self.buf, self.t, self.snap = None, torch.full(shape, fill, dtype=tdt, device=dev()), None
        if data is not None:
            self.t.copy_(data.to(tdt))

    def intact(self):
        return self.buf is None or guards_intact(self.buf, self.snap, self.n)


def _nt_inputs(dt, M, N, K):
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    r = lambda *s, scale=1.0: OB.rnd((torch.randn(*s, generator=g) * scale).double(), dt)
    A, B = r(M, K, scale=0.5), r(N, K, scale=0.05)
    bias = torch.randn(N, generator=g)
    return A, B, bias, r(M, N), r(M, N)


def _variant_kw(variant, bias, resid, mulg, aux):
    kw = dict(bias=None, act=0, aux=None, mulg=None, p=0.0, resid=None, f32=0)
    if variant == "bias":
        kw.update(bias=bias)
    if variant == "bias_gelu_aux":
        kw.update(bias=bias, act=1, aux=aux)
    if variant == "bias_drop_resid":
        kw.update(bias=bias, p=0.1, resid=resid)
    if variant == "mulgrad_resid":
        kw.update(mulg=mulg, resid=resid)
    if variant == "bias_tanh_f32":
        kw.update(bias=bias, act=2, f32=1)
    if variant == "plain_f32":
        kw.update(f32=1)
    return kw


def _run_nt(dt, M, N, K, slow, expect=None, guard=False, variants=VARIANTS, off=None, family=""):
    """every variant of one (dtype, shape, slow): C and aux pre-filled with NaN, C / aux per element, dropped elements exactly the residual, the reported
    path (`expect(variant, path)` asserts it).  off = "A" | "B" | "C" | "bias": that buffer starts one element past a 16-byte boundary."""
    code, tdt = DT[dt]
    A, B, bias, resid, mulg = _nt_inputs(dt, M, N, K)
    where = _where(M, N)
    pr = OB.gemm_nt_products(A.to(where), B.to(where), dt)
    w = lambda t: None if t is None else t.to(where)

    def dbuf(x64, shape, tdt_, shifted):          # operand buffers: guarded, or shifted by one element
        if not shifted:
            return _Buf(shape, tdt_, data=x64, guard=guard)
        b = _Buf((shape[0] * shape[1] + 8,), tdt_)
        b.t = b.t[1:1 + shape[0] * shape[1]].view(*shape)
        b.t.copy_(x64.to(tdt_))
        return b
    Ad, Bd = dbuf(A, (M, K), tdt, off == "A"), dbuf(B, (N, K), tdt, off == "B")
    Rd, Ud = _Buf((M, N), tdt, data=resid, guard=guard), _Buf((M, N), tdt, data=mulg, guard=guard)
    biasd = torch.zeros(N + 4, device=dev())[1:N + 1] if off == "bias" else torch.zeros(N, device=dev())
    biasd.copy_(bias)
    ms, paths = [], {}
    for variant in variants:
        f32 = variant in ("bias_tanh_f32", "plain_f32")
        ctd = torch.float32 if (f32 or dt == "x3") else tdt
        if off == "C":
            Cd = _Buf((M * N + 8,), ctd)
            Cd.t = Cd.t[1:1 + M * N].view(M, N)
        else:
            Cd = _Buf((M, N), ctd, guard=guard)
        auxd = _Buf((M, N), tdt, guard=guard)
        kw = _variant_kw(variant, biasd, Rd.t, Ud.t, auxd.t)
        call("mmhip_op_gemm_nt", code, ptr(Ad.t), K, ptr(Bd.t), K, ptr(Cd.t), N, M, N, K, ptr(kw["bias"]), kw["act"], ptr(kw["aux"]), N,
             ptr(kw["mulg"]), N, kw["p"], SEED, SID, ptr(kw["resid"]), N, kw["f32"], slow, stream())
        path = _lib.last_gemm_path(0)
        torch.cuda.synchronize()
        paths[variant] = path
        if expect is not None:
            expect(variant, path)
        keep, scale = (None, 1.0) if kw["p"] == 0 else keep_mask((M, N), SID, SEED, kw["p"])
        ref, b, pre, pb = OB.gemm_nt_reference(None, None, dt, bias=None if kw["bias"] is None else w(bias), act=kw["act"], mulg=None if kw["mulg"] is None else w(mulg),
                                               keep=w(keep), scale=scale, resid=None if kw["resid"] is None else w(resid), out="f32" if f32 else "t", products=pr)
        got = Cd.t if where.type == "cuda" else Cd.t.cpu()
        ms.append(_check(got, ref, b, f"C {variant} {dt} {M}x{N}x{K} slow={slow} path={path}"))
        if kw["aux"] is not None:
            ms.append(_check(auxd.t if where.type == "cuda" else auxd.t.cpu(), pre, pb, f"aux {dt} {M}x{N}x{K} slow={slow} path={path}"))
        else:
            assert torch.isnan(auxd.t).all(), "aux written although not asked for"
        if keep is not None:
            z = (got.double() - w(resid)) == 0
            kp = w(keep)
            assert z[~kp].all(), "a dropped element is not exactly the residual"
            if M * N >= 4096:          # kept values below half an output ulp of the residual also read as dropped: at most 1 % at these scales (test_op_bounds_cpu.py)
                assert (z & kp).double().mean().item() <= 0.01
        for bb in (Ad, Bd, Rd, Ud, Cd, auxd):
            assert bb.intact(), f"guard band overwritten ({variant})"
    print(f"MARGIN gemm_nt{family} {dt} {M}x{N}x{K} slow={slow} tile={paths[variants[0]][1]} family={paths[variants[0]][0]} worst={max(ms):.4f}")
    return paths


def _expect_forced(dt, M, N, K, slow):
    tile = slow >> 4

    def expect(variant, path):
        what = (dt, M, N, K, slow, variant, path)
        if slow & 1:
            assert path[0] == _lib.NT_GENERIC, what
        elif tile:
            assert path[0] == TILE_FAMILY[tile] and path[1] == tile, what
            ntiles = ((M + TILE_BM[tile] - 1) // TILE_BM[tile]) * (N // TILE_BN[tile])
            assert path[5] == ntiles, what
            if tile in (15, 16, 18):          # persistent: one workgroup per CU, the loop runs on when there are more tiles than that
                assert path[4] == min(ntiles, 256) and path[3] == (1 if ntiles > 256 else 0), what
            if TILE_FAMILY[tile] == 3:        # epilogue class of the deep-pipelined kernel
                assert path[2] == {"plain": 0, "bias_gelu_aux": 1, "bias_drop_resid": 0, "mulgrad_resid": 2, "bias_tanh_f32": 3, "plain_f32": 3, "bias": 0}[variant], what
        elif (M, N, K) in DEFAULT_PATH:
            fam, t, multi = DEFAULT_PATH[(M, N, K)]
            assert path[0] == fam and path[1] == t and (multi is None or path[3] == multi), what
        else:
            assert path[0] in (_lib.NT_TILE, _lib.NT_DEEP), what
    return expect


NT_CASES = [(256, 256, 128, 0), (200, 128, 64, 0), (1000, 768, 768, 0), (8192, 2304, 768, 0),
            (512, 768, 3072, 0), (96, 48, 40, 1), (64, 768, 768, 0),
            (1000, 768, 768, 96), (8192, 2304, 768, 96), (300, 192, 128, 96),
            (300, 128, 128, 144), (8192, 3072, 768, 144), (1000, 768, 2304, 144),
            (200, 96, 64, 160), (8192, 768, 768, 160), (1000, 2304, 768, 160), (300, 480, 128, 0),
            (300, 96, 64, 192), (8192, 768, 3072, 192), (1000, 2304, 768, 192),
            (200, 256, 64, 208), (1000, 768, 768, 208), (8192, 2304, 768, 208), (300, 512, 128, 208),
            (200, 128, 64, 224), (1000, 768, 768, 224), (8192, 2304, 768, 224), (12608, 768, 3072, 224), (300, 384, 192, 224),
            (8192, 3072, 768, 240), (12608, 2304, 768, 240), (8192, 3072, 64, 240), (70000, 256, 128, 240),
            (8192, 3072, 768, 256), (8192, 768, 3072, 256), (12608, 2304, 768, 256), (16384, 768, 2304, 256),
            (40000, 128, 64, 256), (35000, 128, 192, 256),
            (200, 192, 64, 272), (1000, 768, 768, 272), (8192, 3072, 768, 272), (12608, 768, 3072, 272), (300, 384, 128, 272),
            (8192, 3072, 768, 288), (12608, 768, 768, 288), (8192, 3072, 64, 288), (70000, 192, 128, 288), (16384, 2304, 192, 288),
            (256, 256, 320, 208), (256, 128, 320, 224), (256, 192, 320, 272), (35000, 256, 192, 240), (35000, 384, 192, 288),
            (4096, 768, 3072, 336), (1152, 768, 3072, 336), (200, 128, 64, 336), (300, 384, 192, 336), (4096, 768, 2304, 0),
            (12608, 2304, 768, 0), (12608, 768, 768, 0)]          # the last two: the image-tower shapes on the launcher's own choice


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,K,slow", NT_CASES)
def test_gemm_nt_per_element(dt, M, N, K, slow):
    """the cases of test_gpu_ops.py::test_gemm_nt_epilogues (and the 12608-row shapes on default dispatch), six epilogue variants each: per element against
    op_bounds.gemm_nt_reference, the tile / family the case is named for asserted through mmhip_op_last_gemm_path"""
    _run_nt(dt, M, N, K, slow, expect=_expect_forced(dt, M, N, K, slow))


# parity mode: family by the launcher's rules (x3.hip launch_gemm_nt_x3): 7 = operand planes copied to scratch, then the deep-pipelined tile (M > 128, N % 128 == 0,
# K % 64 == 0); 6 = few rows, K over the waves (M <= 128, K % 128 == 0, N % 16 == 0); 5 = the direct 128 x 128 kernel; 1 = generic (K % 32 != 0)
X3_NT_CASES = [(256, 256, 128, 7), (200, 128, 64, 7), (1000, 768, 768, 7), (96, 48, 40, 1), (8192, 2304, 768, 7), (64, 768, 3072, 6), (300, 132, 96, 5), (130, 512, 768, 7),
               (12608, 768, 3072, 7), (700, 384, 192, 7), (64, 3072, 768, 6), (128, 768, 768, 6), (100, 176, 256, 6), (5, 16, 128, 6), (128, 2304, 3072, 6), (100, 128, 96, 5)]


@pytest.mark.parametrize("M,N,K,family", X3_NT_CASES)
def test_x3_gemm_nt_per_element(M, N, K, family):
    def expect(variant, path):
        assert path[0] == family, (M, N, K, variant, path)
        if (M, N, K) == (12608, 768, 3072):          # 200 tiles of 256 x 192 fill the chip best: persistent, one tile per workgroup
            assert path[1] == 18 and path[3] == 0, path
    _run_nt("x3", M, N, K, 0, expect=expect, guard=M <= 1000)


def _edge_shapes(tile):
    """K in {1, 2, depth, depth + 1} k-tiles x M in {1, BM - 1, BM + 1}, N alternating between one tile and nine (the 5 + 4 column groups of gemm8.hip): every
    pair of values of two of the three sizes occurs"""
    bm, bn, d = TILE_BM[tile], TILE_BN[tile], TILE_DEPTH[tile]
    return [(m, bn * (9 if (ki + mi) % 2 else 1), 64 * kt) for ki, kt in enumerate(sorted({1, 2, d, d + 1})) for mi, m in enumerate((1, bm - 1, bm + 1))]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("tile", sorted(TILE_FAMILY))
def test_gemm_nt_tile_edges(dt, tile):
    """per tile code: K of one and two k-tiles, of the ring depth and one more (the pipeline prologue deeper than, equal to, shorter than the loop), M = 1 and one
    off the tile edge on either side, N one tile and nine tiles wide -- every buffer inside guard bands"""
    for M, N, K in _edge_shapes(tile):
        _run_nt(dt, M, N, K, tile << 4, expect=_expect_forced(dt, M, N, K, tile << 4), guard=True, family="_edge")
    # a code no launcher has (20 was the 4-deep ring, TN variant 2 its counterpart): refused, not run on some other kernel
    code, tdt = DT[dt]
    A, B, Cd = torch.zeros(128, 64, dtype=tdt, device=dev()), torch.zeros(128, 64, dtype=tdt, device=dev()), torch.zeros(128, 128, device=dev())
    lib = _lib.lib()
    assert lib.mmhip_op_gemm_nt(code, ptr(A), 64, ptr(B), 64, ptr(Cd), 128, 128, 128, 64, None, 0, None, 0, None, 0, 0.0, 0, 0, None, 0, 1, 20 << 4, stream()) == -1
    assert lib.mmhip_op_gemm_tn(code, ptr(A), 64, ptr(B), 64, ptr(Cd), 64, 128, 64, 64, 0, 2 << 4, None, stream()) == -1


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("M,N,K", [(64, 768, 3072), (128, 768, 1536), (5, 128, 1536)])
def test_gemm_nt_splitk(dt, M, N, K):
    """<= 128 rows, K >= 1536 and a multiple of 384: K / 384 slices side by side, then splitk_finish_kernel with the run-time epilogue (gemm.hip splitk_slices);
    the op entry supplies the workspace.  tanh is outside the rule and must take another kernel."""
    def expect(variant, path):
        if variant == "bias_tanh_f32":
            assert path[0] in (_lib.NT_TILE, _lib.NT_DEEP), (variant, path)
        else:
            assert path[0] == _lib.NT_SPLITK and path[1] == K // 384, (variant, path)
    _run_nt(dt, M, N, K, 0, expect=expect, guard=True, variants=("bias",) + VARIANTS, family="_splitk")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("off", ["A", "B", "C", "bias"])
def test_gemm_nt_unaligned_falls_back(dt, off):
    """an operand, C or the bias one element past a 16-byte boundary with the deep-pipelined 256 x 128 tile forced: nt_fast_ok fails, the generic kernel runs
    (a misaligned bias only where there is a bias: the other variants keep the forced tile)"""
    def expect(variant, path):
        generic = off != "bias" or variant.startswith("bias")
        assert path[0] == (_lib.NT_GENERIC if generic else _lib.NT_DEEP), (off, variant, path)
        if not generic:
            assert path[1] == 14, path
    _run_nt(dt, 300, 256, 128, 224, expect=expect, off=off, family="_unaligned")


# ---------------------------------------------------------------------------------------------------------------- TN
def _tn_inputs(dt, M, Nn, Nc, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    A = OB.rnd((torch.randn(M, Nn, generator=g) * 0.1).double(), dt)
    B = OB.rnd((torch.randn(M, Nc, generator=g) * 0.5).double(), dt)
    return A, B, g


def _tn_check(dt, A, B, Cd, csd, C0, cs0, what, ms):
    where = _where(A.shape[0])
    w = lambda t: None if t is None else t.to(where)
    ref, b, cs, csb = OB.gemm_tn_reference(w(A), w(B), dt, w(C0), w(cs0))
    ms.append(_check(Cd if where.type == "cuda" else Cd.cpu(), ref, b, "C " + what))
    if csd is not None:
        ms.append(_check(csd if where.type == "cuda" else csd.cpu(), cs, csb + 1e-300, "column sums " + what))


def _expect_tn(dt, M, Nn, Nc, slow):
    """(family bits, variant) by launch_gemm_tn's rules"""
    if dt == "x3":
        split = not slow and M % 64 == 0 and Nn % 256 == 0 and Nc % 128 == 0
        return (_lib.TN_TILE | _lib.TN_X3_SPLIT, 4) if split else (_lib.TN_X3_DIRECT, 0)
    v = (slow >> 4) or 4
    if v == 4 and Nn % 256:
        v = 1
    fast = not (slow & 1) and M % 64 == 0 and Nn % (256 if v == 4 else 128) == 0 and Nc % 128 == 0
    return (_lib.TN_TILE, v) if fast else (_lib.TN_GENERIC, 0)


def _run_tn(dt, M, Nn, Nc, slow, expect, with_cs=True, pad=False, family=""):
    """accumulate 0 (C and the column sums pre-filled with NaN), accumulate 1 onto that result, accumulate 0 with NULL column sums (left untouched);
    pad: lda = Nn + 8, ldb = Nc + 8, ldc = Nc + 16 with NaN in the operand pads and a sentinel in C's"""
    code, tdt = DT[dt]
    A, B, _ = _tn_inputs(dt, M, Nn, Nc, M + Nn)
    lda, ldb, ldc = (Nn + 8, Nc + 8, Nc + 16) if pad else (Nn, Nc, Nc)
    Ad, Bd = _Buf((M, lda), tdt, guard=True), _Buf((M, ldb), tdt, guard=True)
    Ad.t[:, :Nn] = A.to(tdt).to(dev())
    Bd.t[:, :Nc] = B.to(tdt).to(dev())
    Cd, csd = _Buf((Nn, ldc), torch.float32, guard=True), _Buf((Nn,), torch.float32, guard=True)
    if pad:
        Cd.t[:, Nc:] = 5.0
    ms = []

    def go(acc, cs):
        call("mmhip_op_gemm_tn", code, ptr(Ad.t), lda, ptr(Bd.t), ldb, ptr(Cd.t), ldc, M, Nn, Nc, acc, slow, ptr(cs), stream())
        path = _lib.last_gemm_path(1)
        torch.cuda.synchronize()
        assert (path[0], path[1]) == expect, (dt, M, Nn, Nc, slow, path)
        assert all(b.intact() for b in (Ad, Bd, Cd, csd)) and (not pad or (Cd.t[:, Nc:] == 5).all()), "written outside C"
        return path
    cs = csd.t if with_cs else None
    go(0, cs)
    _tn_check(dt, A, B, Cd.t[:, :Nc], cs, None, None, "accumulate 0", ms)
    C1, cs1 = Cd.t[:, :Nc].clone(), (None if cs is None else cs.clone())
    go(1, cs)
    _tn_check(dt, A, B, Cd.t[:, :Nc], cs, C1, cs1, "accumulate 1", ms)
    cs2 = csd.t.clone()
    path = go(0, None)
    _tn_check(dt, A, B, Cd.t[:, :Nc], None, None, None, "NULL column sums", ms)
    assert torch.equal(csd.t.view(torch.int32), cs2.view(torch.int32)), "column sums touched although NULL"
    print(f"MARGIN gemm_tn{family} {dt} {M}x{Nn}x{Nc} slow={slow} family={path[0]} variant={path[1]} worst={max(ms):.4f}")


TN_CASES = [(64, 128, 128, 0), (256, 256, 384, 0), (8192, 768, 768, 0), (1024, 2304, 768, 0), (96, 40, 72, 1), (64, 128, 128, 16), (256, 256, 384, 16)]
X3_TN_CASES = [(64, 128, 128), (256, 256, 384), (8192, 768, 768), (1024, 2304, 768), (96, 40, 72), (4, 768, 3072), (100, 768, 768)]


@pytest.mark.parametrize("dt,M,Nn,Nc,slow", [(dt, *c) for dt in ("bf16", "f16") for c in TN_CASES] + [("x3", *c, 0) for c in X3_TN_CASES])
def test_gemm_tn_per_element(dt, M, Nn, Nc, slow):
    _run_tn(dt, M, Nn, Nc, slow, _expect_tn(dt, M, Nn, Nc, slow))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("variant", [1, 4])
@pytest.mark.parametrize("M,Nn,Nc", [(256, 256, 384), (192, 384, 256)])
def test_gemm_tn_variants(dt, variant, M, Nn, Nc):
    """slow >> 4 picks the tile kernel: 1 = 128x128 2-stage, 4 = role-specialised 256x128;
    with Nn % 256 == 128 the 256-row variant 4 falls back to 1 -- seen through the path report"""
    want = 1 if (variant == 4 and Nn % 256) else variant
    assert _expect_tn(dt, M, Nn, Nc, variant << 4) == (_lib.TN_TILE, want)
    _run_tn(dt, M, Nn, Nc, variant << 4, (_lib.TN_TILE, want), family="_variant")


@pytest.mark.parametrize("dt", ["bf16", "f16", "x3"])
@pytest.mark.parametrize("M,Nn,Nc,pad", [(100, 256, 128, False), (80, 3, 768, False), (144, 768, 4, False), (80, 4, 768, False), (64, 128, 3, False),
                                         (256, 256, 384, True), (96, 40, 72, True)])
def test_gemm_tn_edges(dt, M, Nn, Nc, pad):
    """M % 64 != 0 (generic / parity direct), few-column problems (Nn or Nc in {3, 4}; the generic column sums need Nn % 4 == 0), and leading dimensions wider
    than the matrices with NaN in the operand pads and a sentinel in C's pad"""
    _run_tn(dt, M, Nn, Nc, 0, _expect_tn(dt, M, Nn, Nc, 0), with_cs=Nn % 4 == 0, pad=pad, family="_edge")


def _run_tn_group(dt, shapes, expect, family):
    code, tdt = DT[dt]
    g = torch.Generator(device="cpu").manual_seed(11)
    arr = (_lib.TNProblem * len(shapes))()
    held = []
    for i, (M, Nn, Nc) in enumerate(shapes):
        A = OB.rnd((torch.randn(M, Nn, generator=g) * 0.1).double(), dt)
        B = OB.rnd((torch.randn(M, Nc, generator=g) * 0.5).double(), dt)
        C0 = torch.randn(Nn, Nc, generator=g)
        cs0 = torch.randn(Nn, generator=g) if Nn % 4 == 0 else None
        Ad, Bd = A.to(tdt).to(dev()), B.to(tdt).to(dev())
        Cd, csd = _Buf((Nn, Nc), torch.float32, data=C0, guard=True), (None if cs0 is None else _Buf((Nn,), torch.float32, data=cs0, guard=True))
        arr[i] = _lib.TNProblem(Ad.data_ptr(), Bd.data_ptr(), Cd.t.data_ptr(), M, Nn, Nc, Nn, Nc, Nc, None if csd is None else csd.t.data_ptr())
        held.append((A, B, C0, cs0, Ad, Bd, Cd, csd))
    call("mmhip_op_gemm_tn_group", code, C.cast(arr, C.c_void_p), len(shapes), 1, stream())
    path = _lib.last_gemm_path(1)
    torch.cuda.synchronize()
    expect(path)
    ms = []
    for (A, B, C0, cs0, Ad, Bd, Cd, csd), shp in zip(held, shapes):
        assert Cd.intact() and (csd is None or csd.intact()), shp
        _tn_check(dt, A, B, Cd.t, None if csd is None else csd.t, C0, cs0, f"group {shp}", ms)
    print(f"MARGIN gemm_tn_group{family} {dt} problems={len(shapes)} path={path} worst={max(ms):.4f}")


GROUP_SHAPES = [(4096, 768, 768), (4096, 3072, 768), (1152, 768, 2048), (4096, 768, 3072), (80, 3, 768), (144, 768, 4), (4096, 2304, 768), (1152, 768, 768),
                (256, 256, 128), (4096, 768, 768), (4096, 768, 768)]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gemm_tn_group_per_element(dt):
    """the group of test_gpu_ops.py::test_gemm_tn_group_matches_single_problems (accumulate onto non-zero C and column sums): nine problems on the tile kernel
    -- one more than a launch takes -- and two generic ones.  The launcher's Nn % 256 rule looks at EVERY problem of the call, the generic ones included: the
    3-row problem moves the whole group from the default role-specialised 256x128 variant (4) to 128x128 (1) -- asserted as the code has it."""
    mg = _lib.lib().mmhip_tn_max_group()

    def expect(path):
        assert path[0] == (_lib.TN_TILE | _lib.TN_GENERIC) and path[1] == 1 and path[2] == 9 and path[3] == 2 and path[4] == (9 + mg - 1) // mg, path
    _run_tn_group(dt, GROUP_SHAPES, expect, "")


@pytest.mark.parametrize("dt", ["bf16", "f16", "x3"])
def test_gemm_tn_group_flushes_in_the_middle(dt):
    """more fast problems than one launch of the grouped kernel takes (mmhip_tn_max_group(), read from the library) plus a generic one in between: the 16-bit
    launcher flushes a full group and goes on; the parity launcher sends the first mmhip_tn_max_group() through the scratch-split form and the rest through
    its direct kernel"""
    mg = _lib.lib().mmhip_tn_max_group()
    cyc = [(64, 256, 128), (128, 256, 256), (64, 512, 128)]
    shapes = [cyc[i % 3] for i in range(mg + 3)]
    shapes.insert(mg // 2, (100, 256, 128))          # M % 64 != 0: generic / parity direct, and Nn % 256 == 0 keeps the group on variant 4

    def expect(path):
        if dt == "x3":
            assert path[0] == (_lib.TN_TILE | _lib.TN_X3_SPLIT | _lib.TN_X3_DIRECT) and path[2] == mg and path[6] == mg and path[5] == 4 and path[4] == 1, path
        else:
            assert path[0] == (_lib.TN_TILE | _lib.TN_GENERIC) and path[1] == 4 and path[2] == mg + 3 and path[3] == 1 and path[4] == 2, path
    _run_tn_group(dt, shapes, expect, "_flush")


# ---------------------------------------------------------------------------------------------------------------- LayerNorm, column sums
@pytest.mark.parametrize("dt", ["bf16", "f16", "x3"])
@pytest.mark.parametrize("rows,width", [(37, 768), (8192, 768), (130, 1024), (1, 768), (5, 768), (257, 768), (1, 4), (5, 4), (257, 4)])
def test_layernorm_per_element(dt, rows, width):
    """forward (y, mean, rstd: op_bounds.ln_bounds with the type's u_out) and backward on the kernel's own saved statistics (dx + dres, dgamma, dbeta:
    op_bounds.ln_bwd_reference; the residual add and the store add (U_32 + u_out) |dx + dres|).  Every fourth row has mean 1e3 and unit spread, row 2 is constant
    (variance 0: rstd = 1 / sqrt(eps), y = beta, xhat = 0); outputs pre-filled with NaN inside guard bands."""
    code, tdt = DT[dt]
    eps = 1e-5
    u = OB.FMT[dt].u_out
    g = torch.Generator(device="cpu").manual_seed(rows + width)
    x = OB.ln_edge_rows(rows, width, g, dt)
    gamma, beta = 1 + 0.1 * torch.randn(width, generator=g), 0.1 * torch.randn(width, generator=g)
    dy, dres = OB.rnd(torch.randn(rows, width, generator=g).double(), dt), OB.rnd(torch.randn(rows, width, generator=g).double(), dt)
    X, DY, DR = (_Buf((rows, width), tdt, data=t, guard=True) for t in (x, dy, dres))
    G, Be = gamma.to(dev()), beta.to(dev())
    Y, mean, rstd = _Buf((rows, width), tdt, guard=True), _Buf((rows,), torch.float32, guard=True), _Buf((rows,), torch.float32, guard=True)
    call("mmhip_op_layernorm_fwd", code, ptr(X.t), ptr(Y.t), ptr(G), ptr(Be), ptr(mean.t), ptr(rstd.t), rows, width, eps, stream())
    torch.cuda.synchronize()
    ref, rmean, rrstd = OB.ln_reference(x, gamma, beta, eps)
    yb, mb, rb = OB.ln_bounds(x, gamma, beta, eps, u)
    m = (assert_close_elementwise(Y.t, ref, yb, "y"), assert_close_elementwise(mean.t, rmean, mb, "mean"), assert_close_elementwise(rstd.t, rrstd, rb, "rstd"))
    assert all(b.intact() for b in (X, Y, mean, rstd))
    print(f"MARGIN ln_fwd {dt} rows={rows} width={width} y={m[0]:.4f} mean={m[1]:.4f} rstd={m[2]:.4f}")
    DX = _Buf((rows, width), tdt, guard=True)
    dg, db = _Buf((width,), torch.float32, fill=0.0, guard=True), _Buf((width,), torch.float32, fill=0.0, guard=True)
    call("mmhip_op_layernorm_bwd", code, ptr(DY.t), ptr(X.t), ptr(G), ptr(mean.t), ptr(rstd.t), ptr(DX.t), ptr(DR.t), ptr(dg.t), ptr(db.t), rows, width, stream())
    torch.cuda.synchronize()
    dx, dx_e, _, dgam, dgam_b, dbet, dbet_b = OB.ln_bwd_reference(dy, x, gamma, mean.t.cpu(), rstd.t.cpu())
    tot = dx + dres
    m = (assert_close_elementwise(DX.t, tot, OB.SLACK * (dx_e + (OB.U_32 + u) * tot.abs()), "dx + dres"),
         assert_close_elementwise(dg.t, dgam, dgam_b, "dgamma"), assert_close_elementwise(db.t, dbet, dbet_b, "dbeta"))
    assert all(b.intact() for b in (DY, DR, DX, dg, db, X, mean, rstd))
    print(f"MARGIN ln_bwd {dt} rows={rows} width={width} dx={m[0]:.4f} dgamma={m[1]:.4f} dbeta={m[2]:.4f}")


@pytest.mark.parametrize("dt", ["bf16", "f16", "x3"])
@pytest.mark.parametrize("rows", [1, 1000, 8192])
@pytest.mark.parametrize("cols,ld", [(2304, 2304), (260, 268), (4, 12)])
def test_colsum_per_element(dt, rows, cols, ld):
    """out[c] += sum_r x[r][c] in bf16, f16 and fp32, leading dimension wider than the matrix (NaN pads), column counts off the 256-column block:
    rows U_32 sum |x|, times SLACK (op_bounds.colsum_reference)"""
    code, tdt = DT[dt]
    g = torch.Generator(device="cpu").manual_seed(rows + cols)
    x = OB.rnd(torch.randn(rows, cols, generator=g).double(), dt)
    X = _Buf((rows, ld), tdt, guard=True)
    X.t[:, :cols] = x.to(tdt).to(dev())
    out = _Buf((cols,), torch.float32, fill=0.0, guard=True)
    call("mmhip_op_colsum", code, ptr(X.t), rows, cols, ld, ptr(out.t), stream())
    torch.cuda.synchronize()
    ref, b = OB.colsum_reference(x)
    m = assert_close_elementwise(out.t, ref, b + 1e-300, "column sums")
    assert out.intact() and X.intact()
    print(f"MARGIN colsum {dt} rows={rows} cols={cols} ld={ld} worst={m:.4f}")


@pytest.mark.parametrize("code", [3, 7, -1])
def test_colsum_rejects_other_dtype_codes(code):
    """MMHIP_PAIR and unknown codes: MMHIP_E_INVALID before any launch, out untouched (the launcher would read them as fp32)"""
    x = torch.randn(64, 256, device=dev())
    out = torch.full((256,), 5.0, device=dev())
    rc = _lib.lib().mmhip_op_colsum(code, ptr(x), 64, 256, 256, ptr(out), stream())
    torch.cuda.synchronize()
    assert rc == -1 and (out == 5).all()
