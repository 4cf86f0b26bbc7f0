"""-m gpu: the three BEiT operators through their C entry points, per element against fp64 on the very values the kernel reads, with the bounds
derived in tests/beit_ref.py (sums of named rounding terms on top of tests/op_bounds.py; tests/test_beit_cpu.py shows that a missing, transposed or
wrong-head bias leaves them by far).

  mmhip_op_attn_fwd_bias     S = 5 (one tile, the 2 x 2 window), 37 (two tiles with a tail), 197 (seven tiles, the real window), 129 (the <4, 4> / <7, 8>
                             edge); posts = 2, heads = 2; bf16, f16, parity mode on fp32 tensors ("x3") and on plane pairs ("pair"); bias values of the
                             order of the scores: random, asymmetric in (query, key), different per head; row stride = S rounded up to 4 and wider
  mmhip_op_beit_bias_image   bit-exact against the gather on the CPU for 2 x 2, 4 x 4 and 14 x 14 windows
  mmhip_op_patch_mean_ln     rows = 5, 37, 197 at widths 128 and 768, every dtype
  refusals                   the launcher answers before any launch and leaves the outputs untouched
Every case prints its margin max(|err| / bound) (pytest -s); profiles/op_test_margins.md holds the table."""
import ctypes as C

import pytest
import torch

import beit_ref as R
import op_bounds as OB

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gpu_util import dev, ptr, stream, assert_close_elementwise, guarded, guards_intact
    from smtc_amd import _lib

CODE = {"bf16": 0, "f16": 1, "x3": 2, "pair": 3}
TDT = {"bf16": torch.bfloat16, "f16": torch.float16, "x3": torch.float32, "pair": torch.bfloat16}
DTS = ["bf16", "f16", "x3", "pair"]
POSTS, HEADS = 2, 2


def put(x64, dt):
    if dt == "pair":
        hi, lo = OB.split_pair(x64)
        return torch.cat([hi, lo], dim=1).contiguous().to(dev())
    return x64.to(TDT[dt]).contiguous().to(dev())


def get(t, dt, W):
    t = t.cpu()
    if dt != "pair":
        return t.double()
    hi, lo = t[:, :W], t[:, W:]
    assert OB.pair_hi_is_nearest(hi, lo).all(), "hi plane is not the value rounded to bf16"
    return hi.double() + lo.double()


def run_attn(dt, S, kind, ld=None):
    H = HEADS * 64
    ld = (S + 3) // 4 * 4 if ld is None else ld
    qkv64, bias = R.attn_bias_inputs(dt, POSTS, S, HEADS, seed=100 * S + len(kind), kind=kind)
    r = R.attn_bias_reference(qkv64, bias, POSTS, S, HEADS)
    ctx_b, lse_b = R.attn_bias_bounds(r, bias, dt, S)
    qkv, b2d = put(qkv64, dt), R.pad_bias(bias, ld).to(dev())
    cbuf, ctx, csnap = guarded((POSTS * S, 2 * H if dt == "pair" else H), TDT[dt], float("nan"))
    lbuf, lse, lsnap = guarded((POSTS, HEADS, S), torch.float32, float("nan"))
    rc = _lib.lib().mmhip_op_attn_fwd_bias(CODE[dt], ptr(qkv), ptr(b2d), ld, ptr(ctx), ptr(lse), POSTS, S, HEADS, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guards_intact(cbuf, csnap, ctx.numel()) and guards_intact(lbuf, lsnap, lse.numel()), "write outside ctx / lse"
    m1 = assert_close_elementwise(get(ctx, dt, H), OB.to_rows(r.ctx), OB.to_rows(ctx_b), f"ctx {dt} S={S} {kind}")
    m2 = assert_close_elementwise(lse, r.lse, lse_b, f"lse {dt} S={S} {kind}")
    # the bias matters at this size: without it the reference is many bounds away
    r0 = R.attn_bias_reference(qkv64, torch.zeros_like(bias), POSTS, S, HEADS)
    assert ((r0.ctx - r.ctx).abs() > 10 * ctx_b).float().mean().item() > 0.5
    print(f"MARGIN attn_fwd_bias {dt} posts={POSTS} S={S} heads={HEADS} bias={kind} ld={ld} ctx={m1:.4f} lse={m2:.4f}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("S", [5, 37, 129, 197])
def test_attention_forward_with_bias(dt, S):
    run_attn(dt, S, "random")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", ["asym", "perhead"])
def test_attention_forward_with_asymmetric_and_per_head_bias(dt, kind):
    """asym: bias[q, k] = -bias[k, q], a transposed read is wrong everywhere; perhead: the heads' biases differ in sign and size"""
    run_attn(dt, 37, kind)
    run_attn(dt, 197, kind, ld=208)          # a row stride wider than S rounded up to 4


def test_attention_bias_refusals_leave_the_outputs_untouched():
    S, H = 37, HEADS * 64
    qkv64, bias = R.attn_bias_inputs("bf16", POSTS, S, HEADS, seed=1)
    qkv = put(qkv64, "bf16")
    b2d = torch.zeros(HEADS * S * 48 + 8, dtype=torch.float32, device=dev())
    ctx = torch.full((POSTS * S, H), 7.0, dtype=torch.bfloat16, device=dev())
    lse = torch.full((POSTS, HEADS, S), 7.0, dtype=torch.float32, device=dev())
    lib = _lib.lib()
    call = lambda dt, q, b, ld, s: lib.mmhip_op_attn_fwd_bias(dt, ptr(q), b, ld, ptr(ctx), ptr(lse), POSTS, s, HEADS, stream())
    at = lambda off: C.c_void_p(b2d.data_ptr() + off)          # the bias `off` bytes into its allocation
    assert call(0, qkv, at(0), 40, S) == 0                         # the accepted form, for contrast
    torch.cuda.synchronize()
    ctx.fill_(7.0)
    lse.fill_(7.0)
    bad = [call(0, qkv, at(0), 38, S),          # ld_bias % 4 != 0
           call(0, qkv, at(0), 36, S),          # ld_bias < S
           call(0, qkv, at(4), 40, S),          # bias off 16-byte alignment
           call(0, qkv, None, 40, S),           # no bias
           call(7, qkv, at(0), 40, S),          # no such dtype
           call(0, qkv, at(0), 228, 225)]       # no bias instantiation past 224 keys
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in bad), bad
    assert (ctx == 7.0).all() and (lse == 7.0).all()


@pytest.mark.parametrize("W", [2, 4, 14])
def test_bias_image_is_bit_exact(W):
    heads, P = 12 if W == 14 else 2, W * W + 1
    ld = (P + 3) // 4 * 4
    g = torch.Generator().manual_seed(W)
    table = torch.randn((2 * W - 1) ** 2 + 3, heads, generator=g)
    buf, out, snap = guarded((heads, P, ld), torch.float32, float("nan"))
    td = table.to(dev())
    rc = _lib.lib().mmhip_op_beit_bias_image(ptr(td), heads, W, W, ptr(out), ld, stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(buf, snap, out.numel())
    assert torch.equal(out.cpu(), R.bias_image(table, W, W, ld))
    assert _lib.lib().mmhip_op_beit_bias_image(ptr(td), heads, W, W, ptr(out), P - 1, stream()) == -1


@pytest.mark.parametrize("dt", ["bf16", "f16", "x3"])
@pytest.mark.parametrize("rows", [5, 37, 197])
@pytest.mark.parametrize("width", [128, 768])
def test_patch_mean_ln(dt, rows, width):
    posts = 3
    g = torch.Generator().manual_seed(rows + width)
    x64 = OB.rnd((torch.randn(posts * rows, width, generator=g) * 2 + 0.3).double(), dt)
    x64.view(posts, rows, width)[:, 0] = OB.rnd(torch.full((posts, width), 50.0).double(), dt)          # a CLS row that must not enter the mean
    gamma, beta = 1 + 0.1 * torch.randn(width, generator=g), 0.02 * torch.randn(width, generator=g)
    ref, bound = R.patch_mean_ln_reference(x64, rows, gamma, beta, 1e-12)
    xd, gd, bd = put(x64, dt), gamma.to(dev()), beta.to(dev())          # (held: a temporary's memory would be handed to the next allocation)
    call = lambda r, o: _lib.lib().mmhip_op_patch_mean_ln(CODE[dt], ptr(xd), r, posts, width, ptr(gd), ptr(bd), 1e-12, ptr(o), stream())
    buf, out, snap = guarded((posts, width), torch.float32, float("nan"))
    assert call(rows, out) == 0
    torch.cuda.synchronize()
    assert guards_intact(buf, snap, out.numel())
    m = assert_close_elementwise(out, ref, bound, f"patch_mean_ln {dt} rows={rows} width={width}")
    again = torch.full_like(out, float("nan"))
    assert call(rows, again) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, again)          # fixed summation order: the same bits
    print(f"MARGIN patch_mean_ln {dt} posts={posts} rows={rows} width={width} out={m:.4f}")
    assert call(1, out) == -1
