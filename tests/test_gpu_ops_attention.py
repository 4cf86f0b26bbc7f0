"""-m gpu: mmhip_op_attn_fwd / mmhip_op_attn_bwd in every form (bf16, f16, the parity mode on fp32 tensors "x3", the parity mode on plane pairs
"pair" = MMHIP_PAIR) at every tier edge of the launchers (csrc/attention.hip launch_fwd_d / launch_attn_fwd / launch_attn_bwd, csrc/x3.hip
launch_attn_*_f32) and the production lengths, against fp64 attention on the very values the kernel reads -- PER ELEMENT, with the bounds derived in
tests/op_bounds.py (attn_fwd_bounds / attn_bwd_bounds: sums of named rounding terms, overall factor 2; tests/test_op_bounds_cpu.py shows that an
off-by-one attention leaves them).  Outputs sit between 64-element guard bands inside the test's own allocation and are pre-filled with NaN.

Which kernel a case reaches:  S <= 32 / 64 / 128 / 224 / 288 the one-image tiers (16-bit: also <= 608, <19, 8>); parity 289..768 the chunked
attn_fwd_x3_long_kernel<PAIR>; parity fp32 with S > 768 or a pointer off 16-byte alignment the vector-ALU kernels (bounded as "alu": no operand
split); parity backward: S <= 128 the MFMA kernel, fp32 tensors above that (or unaligned) the ALU kernels.  Every case prints its margin
max(|err| / bound) (pytest -s); profiles/op_test_margins.md holds the table."""
import pytest
import torch

import op_bounds as OB

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gpu_util import dev, ptr, stream, keep_mask, assert_close_elementwise, guarded, guards_intact
    from smtc_amd import _lib

CODE = {"bf16": 0, "f16": 1, "x3": 2, "pair": 3}
TDT = {"bf16": torch.bfloat16, "f16": torch.float16, "x3": torch.float32, "pair": torch.bfloat16}
DTS = ["bf16", "f16", "x3", "pair"]
SEED, SID = 77, 16
FWD_S = [1, 31, 32, 33, 64, 65, 128, 129, 197, 224, 225, 257, 288, 289, 577, 608]


def rc_of(name, *args):
    return getattr(_lib.lib(), name)(*args)


def put(x64, dt, shift=0):
    """fp64 [rows, W] -> device tensor as the form stores it (pair: rows of [hi (W) | lo (W)]); shift: elements to offset the tensor inside its allocation"""
    if dt == "pair":
        hi, lo = OB.split_pair(x64)
        t = torch.cat([hi, lo], dim=1).contiguous()
    else:
        t = x64.to(TDT[dt]).contiguous()
    if not shift:
        return t.to(dev())
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=dev())
    v = buf[shift:shift + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def get(t, dt, W):
    """device tensor -> fp64 [rows, W] on the CPU; pair: hi + lo, after checking that hi alone is the value rounded to bf16 (OB.pair_hi_is_nearest)"""
    t = t.cpu()
    if dt != "pair":
        return t.double()
    hi, lo = t[:, :W], t[:, W:]
    fin = torch.isfinite(hi.float()) & torch.isfinite(lo.float())
    assert OB.pair_hi_is_nearest(hi[fin], lo[fin]).all(), "hi plane is not the value rounded to bf16"
    return hi.double() + lo.double()


def out_buf(rows, W, dt):
    return guarded((rows, 2 * W if dt == "pair" else W), TDT[dt], float("nan"))


def fwd_path(dt, S, aligned=True):
    return "alu" if dt == "x3" and (S > 768 or not aligned) else dt


def bwd_path(dt, S, aligned=True):
    return "alu" if dt == "x3" and (S > 128 or not aligned) else dt


def run_fwd(dt, posts, S, heads, masked, p, shift=0):
    H = heads * 64
    qkv64, _, maskbias = OB.attn_inputs(dt, posts, S, heads, masked, seed=1000 * posts + S)
    keep, scale = (None, 1.0) if p == 0 else keep_mask((posts, heads, S, S), SID, SEED, p)
    r = OB.attn_reference(qkv64, maskbias, posts, S, heads, keep, scale)
    ctx_b, lse_b = OB.attn_fwd_bounds(r, fwd_path(dt, S, not shift), S)
    qkv = put(qkv64, dt, shift)
    mb = None if maskbias is None else maskbias.to(dev())
    cbuf, ctx, csnap = out_buf(posts * S, H, dt)
    lbuf, lse, lsnap = guarded((posts, heads, S), torch.float32, float("nan"))
    rc = rc_of("mmhip_op_attn_fwd", CODE[dt], ptr(qkv), ptr(mb), ptr(ctx), ptr(lse), posts, S, heads, p, SEED, SID, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guards_intact(cbuf, csnap, ctx.numel()) and guards_intact(lbuf, lsnap, lse.numel()), "write outside ctx / lse"
    m1 = assert_close_elementwise(get(ctx, dt, H), OB.to_rows(r.ctx), OB.to_rows(ctx_b), f"ctx {dt} S={S}")
    m2 = assert_close_elementwise(lse, r.lse, lse_b, f"lse {dt} S={S}")
    print(f"MARGIN attn_fwd{'_drop' if p else ''} {dt} posts={posts} S={S} heads={heads} masked={int(masked)} path={fwd_path(dt, S, not shift)} ctx={m1:.4f} lse={m2:.4f}")


def _fwd_cases():
    out = []
    for dt in DTS:
        for S in FWD_S + ([609, 768] if dt in ("x3", "pair") else []) + ([769] if dt == "x3" else []):
            for masked in (False, True):
                out.append((dt, 3, S, 2, masked))
        out += [(dt, 5, 65, 16, True), (dt, 5, 257, 16, True)]
    return out


@pytest.mark.parametrize("dt,posts,S,heads,masked", _fwd_cases())
def test_attention_forward(dt, posts, S, heads, masked):
    """ctx and lse per element (op_bounds.attn_fwd_bounds); masks: post 0 full, post 1 a single key, post 2 one or more whole 32-key tiles (S >= 295:
    a whole 288-key chunk of the long kernel) masked"""
    run_fwd(dt, posts, S, heads, masked, 0.0)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("S", [33, 197, 257, 577, 64, 288])
def test_attention_forward_dropout(dt, S):
    """p = 0.1 at odd S (one hash per element, DROP=1) and even S (one hash per key pair, DROP=2), masks replayed by keep_mask"""
    run_fwd(dt, 3, S, 2, True, 0.1)


def test_attention_forward_unaligned_fp32_takes_the_alu_kernel():
    """parity mode, qkv 4 bytes off 16-byte alignment: the supported vector-ALU fallback (attn_fwd_f32_kernel), with and without dropout"""
    run_fwd("x3", 3, 33, 2, True, 0.0, shift=1)
    run_fwd("x3", 3, 197, 2, True, 0.1, shift=1)


def test_attention_forward_long_alu_kernel_with_dropout():
    """attn_fwd_f32_long_kernel (rows from global memory: S >= 318 on the ALU path) with its dropout branch: unaligned at 577 tokens, aligned at 769"""
    run_fwd("x3", 3, 577, 2, True, 0.1, shift=1)
    run_fwd("x3", 3, 769, 2, True, 0.1)


def run_bwd(dt, posts, S, heads, p, shift=0):
    H = heads * 64
    qkv64, dctx64, maskbias = OB.attn_inputs(dt, posts, S, heads, True, seed=2000 * posts + S, with_dctx=True)
    keep, scale = (None, 1.0) if p == 0 else keep_mask((posts, heads, S, S), SID, SEED, p)
    r = OB.attn_reference(qkv64, maskbias, posts, S, heads, keep, scale, dctx64)
    path = bwd_path(dt, S, not shift)
    bounds = OB.attn_bwd_bounds(r, path, S)
    qkv, dctx, mb = put(qkv64, dt, shift), put(dctx64, dt), maskbias.to(dev())
    ctx = put(OB.to_rows(r.ctx), dt)                 # the backward's saved inputs: the reference's ctx and lse, as stored
    lse = r.lse.float().to(dev()).contiguous()
    gbuf, dqkv, gsnap = out_buf(posts * S, 3 * H, dt)
    rc = rc_of("mmhip_op_attn_bwd", CODE[dt], ptr(qkv), ptr(mb), ptr(ctx), ptr(dctx), ptr(lse), ptr(dqkv), posts, S, heads, p, SEED, SID, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guards_intact(gbuf, gsnap, dqkv.numel()), "write outside dqkv"
    got = get(dqkv, dt, 3 * H)
    ms = []
    for i, (name, ref, b) in enumerate(zip(("dq", "dk", "dv"), (r.dq, r.dk, r.dv), bounds)):
        ms.append(assert_close_elementwise(got[:, i * H:(i + 1) * H], OB.to_rows(ref), OB.to_rows(b), f"{name} {dt} S={S} p={p}"))
    dead = OB.to_rows((~r.live[:, :, 0, :]).unsqueeze(-1).expand_as(r.dk))
    assert (got[:, H:2 * H][dead] == 0).all() and (got[:, 2 * H:][dead] == 0).all(), "masked keys: dk / dv must be exactly 0"
    print(f"MARGIN attn_bwd{'_drop' if p else ''} {dt} posts={posts} S={S} heads={heads} path={path} dq={ms[0]:.4f} dk={ms[1]:.4f} dv={ms[2]:.4f}")


def _bwd_cases():
    out = [(dt, S, p) for dt in DTS for S in (1, 31, 33, 64, 65, 127, 128) for p in (0.0, 0.1)]
    return out + [("x3", S, p) for S in (129, 197, 257) for p in (0.0, 0.1)]


@pytest.mark.parametrize("dt,S,p", _bwd_cases())
def test_attention_backward(dt, S, p):
    """dq, dk, dv per element against fp64 autograd (op_bounds.attn_bwd_bounds), exact zeros on masked keys, dqkv pre-filled with NaN between guard
    bands.  x3 at S > 128: launch_attn_bwd_f32 (attn_bwd_f32_long_kernel)"""
    run_bwd(dt, 3, S, 2, p)


def test_attention_backward_unaligned_fp32_takes_the_alu_kernel():
    run_bwd("x3", 3, 65, 2, 0.1, shift=1)


# ---------------------------------------------------------------------------------------------------------------- host-side rejects
def _reject(rc):
    assert rc == -1 or rc > 0, rc


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_rejected_before_any_launch_16bit(dt):
    """launch_fwd_d has no tier above 608 keys, launch_bwd_d none above 128: both return before a launch; the outputs stay as they were"""
    posts, heads = 1, 1
    for S, bwd in ((609, False), (129, True)):
        qkv = torch.zeros(posts * S, 192, dtype=TDT[dt], device=dev())
        ctx = torch.full((posts * S, 64), 3.0, dtype=TDT[dt], device=dev())
        lse = torch.full((posts, heads, S), 3.0, device=dev())
        dqkv = torch.full((posts * S, 192), 3.0, dtype=TDT[dt], device=dev())
        if bwd:
            _reject(rc_of("mmhip_op_attn_bwd", CODE[dt], ptr(qkv), None, ptr(ctx), ptr(ctx), ptr(lse), ptr(dqkv), posts, S, heads, 0.0, 0, 0, stream()))
        else:
            _reject(rc_of("mmhip_op_attn_fwd", CODE[dt], ptr(qkv), None, ptr(ctx), ptr(lse), posts, S, heads, 0.0, 0, 0, stream()))
        torch.cuda.synchronize()
        assert (ctx == 3).all() and (lse == 3).all() and (dqkv == 3).all()


def test_rejected_before_any_launch_pair():
    """plane pairs have no vector-ALU fallback: S > 768 and a pointer off 16-byte alignment are errors (launch_attn_fwd)"""
    for S, shift in ((769, 0), (33, 1)):
        buf = torch.zeros(S * 384 + 16, dtype=torch.bfloat16, device=dev())
        qkv = buf[shift:shift + S * 384]
        ctx = torch.full((S, 128), 3.0, dtype=torch.bfloat16, device=dev())
        lse = torch.full((1, 1, S), 3.0, device=dev())
        _reject(rc_of("mmhip_op_attn_fwd", 3, ptr(qkv), None, ptr(ctx), ptr(lse), 1, S, 1, 0.0, 0, 0, stream()))
        torch.cuda.synchronize()
        assert (ctx == 3).all() and (lse == 3).all()


@pytest.mark.parametrize("width", [1028, 770])
def test_rejected_before_any_launch_layernorm(width):
    x = torch.zeros(8, width, device=dev())
    y = torch.full((8, width), 3.0, device=dev())
    g = torch.ones(width, device=dev())
    mean = torch.full((8,), 3.0, device=dev())
    _reject(rc_of("mmhip_op_layernorm_fwd", 2, ptr(x), ptr(y), ptr(g), ptr(g), ptr(mean), ptr(mean), 8, width, 1e-5, stream()))
    torch.cuda.synchronize()
    assert (y == 3).all() and (mean == 3).all()
