"""-m gpu: mmhip_op_attn_bwd_long -- the self-attention backward for 129..288 keys (csrc/attention.hip "long backward": a key role and a query role,
every product on MFMA) -- in the four forms of tests/test_gpu_ops_attention.py (bf16, f16, "x3" = parity mode on fp32 tensors, "pair" = plane pairs),
against fp64 autograd on the very values the kernel reads, PER ELEMENT with op_bounds.attn_bwd_bounds.  Here "x3" is bounded as "x3" (three bf16
products), not as "alu": this entry has no vector-ALU kernel.  dqkv sits NaN-filled between guard bands; every element is checked, masked keys must
be exact zeros, the hi plane of a pair must be the value rounded to bf16 (the `get` helper).  Each case prints a MARGIN line (pytest -s).

Sizes: every tile-count step (multiples of 32) and chunk-count step (128 | 129, 256 | 257) of the launcher from both sides, 197 and 257 (ViT-B/16,
CLIP-ViT-L/14 @224).  Mask: live lengths [S, 1, S - 37, 129, 33] (attn_long_cases.live_lengths)."""
import pytest
import torch

import op_bounds as OB
import attn_long_cases as AL
from test_gpu_ops_attention import CODE, TDT, DTS, put, get, out_buf, rc_of, _reject

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from gpu_util import dev, ptr, stream, assert_close_elementwise, guarded, guards_intact

SEED, SID = AL.SEED, AL.SID


def call_long(dt, qkv, mb, ctx, dctx, lse, dqkv, posts, S, heads, p):
    return rc_of("mmhip_op_attn_bwd_long", CODE[dt], ptr(qkv), ptr(mb), ptr(ctx), ptr(dctx), ptr(lse), ptr(dqkv), posts, S, heads, p, SEED, SID, stream())


def run_long(dt, posts, S, heads, p, masked=True, composite=False, twice=False):
    H = heads * 64
    c = AL.case(dt, posts, S, heads, p, masked)
    r = c.r
    qkv, dctx = put(c.qkv64, dt), put(c.dctx64, dt)
    mb = None if c.maskbias is None else c.maskbias.to(dev())
    if composite:          # the forward's own ctx and lse, as it stored them; its bounds enter the backward's
        ctx_b, lse_b = OB.attn_fwd_bounds(r, dt, S)
        cbuf, ctx, csnap = out_buf(posts * S, H, dt)
        lbuf, lse, lsnap = guarded((posts, heads, S), torch.float32, float("nan"))
        rc = rc_of("mmhip_op_attn_fwd", CODE[dt], ptr(qkv), ptr(mb), ptr(ctx), ptr(lse), posts, S, heads, p, SEED, SID, stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert guards_intact(cbuf, csnap, ctx.numel()) and guards_intact(lbuf, lsnap, lse.numel()), "write outside ctx / lse"
        bounds = OB.attn_bwd_bounds(r, dt, S, ctx_err=ctx_b, lse_err=lse_b)
    else:                  # the reference's ctx and lse, as stored
        ctx = put(OB.to_rows(r.ctx), dt)
        lse = r.lse.float().to(dev()).contiguous()
        bounds = OB.attn_bwd_bounds(r, dt, S)
    gbuf, dqkv, gsnap = out_buf(posts * S, 3 * H, dt)
    rc = call_long(dt, qkv, mb, ctx, dctx, lse, dqkv, posts, S, heads, p)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guards_intact(gbuf, gsnap, dqkv.numel()), "write outside dqkv"
    if twice:
        gbuf2, dqkv2, gsnap2 = out_buf(posts * S, 3 * H, dt)
        assert call_long(dt, qkv, mb, ctx, dctx, lse, dqkv2, posts, S, heads, p) == 0
        torch.cuda.synchronize()
        it = torch.int32 if dt == "x3" else torch.int16
        assert guards_intact(gbuf2, gsnap2, dqkv2.numel()) and torch.equal(dqkv.view(it), dqkv2.view(it)), "the same call twice: different bits"
    got = get(dqkv, dt, 3 * H)
    ms = []
    for i, (name, ref, b) in enumerate(zip(("dq", "dk", "dv"), (r.dq, r.dk, r.dv), bounds)):
        ms.append(assert_close_elementwise(got[:, i * H:(i + 1) * H], OB.to_rows(ref), OB.to_rows(b), f"{name} {dt} S={S} p={p}"))
    dead = OB.to_rows((~r.live[:, :, 0, :]).unsqueeze(-1).expand_as(r.dk))
    assert (got[:, H:2 * H][dead] == 0).all() and (got[:, 2 * H:][dead] == 0).all(), "masked keys: dk / dv must be exactly 0"
    kind = "composite" if composite else "twice" if twice else "plain"
    print(f"MARGIN attn_bwd_long{'_drop' if p else ''} {dt} posts={posts} S={S} heads={heads} masked={int(masked)} {kind} dq={ms[0]:.4f} dk={ms[1]:.4f} dv={ms[2]:.4f}")


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", AL.GRID_S)
@pytest.mark.parametrize("dt", DTS)
def test_long_backward(dt, S, p):
    """dq, dk, dv per element, posts 5, heads 2, masked: a full post, a single key, a dead tail tile, posts whose later tiles / chunks hold no live key"""
    run_long(dt, 5, S, 2, p)


@pytest.mark.parametrize("dt", DTS)
def test_long_backward_no_mask(dt):
    """maskbias = NULL (the ViT case)"""
    run_long(dt, 3, 197, 2, 0.0, masked=False)


@pytest.mark.parametrize("dt", DTS)
def test_long_backward_wide(dt):
    """16 heads: the row strides of a 1024-wide tower, and dropout indices beyond one head's S x S block"""
    run_long(dt, 5, 257, 16, 0.1)


@pytest.mark.parametrize("S", [197, 257])
@pytest.mark.parametrize("dt", DTS)
def test_long_backward_after_the_forward_op(dt, S):
    """mmhip_op_attn_fwd (p = 0.1) writes ctx and lse, mmhip_op_attn_bwd_long reads them: a dropout index or an lse unit that differed between the
    forward tier and this backward would leave the bounds"""
    run_long(dt, 5, S, 2, 0.1, composite=True)


@pytest.mark.parametrize("S", [197, 288])
@pytest.mark.parametrize("dt", DTS)
def test_long_backward_same_bits_twice(dt, S):
    run_long(dt, 5, S, 2, 0.1, twice=True)


def _rejected_call(dt, S, off=None):
    """one call with dqkv pre-filled with 3.0; off = (index of the tensor among qkv, ctx, dctx, dqkv; elements to shift it by)"""
    W = 2 if dt == "pair" else 1
    shapes = [(S, 192 * W), (S, 64 * W), (S, 64 * W), (S, 192 * W)]
    bufs, views = [], []
    for i, (rows, cols) in enumerate(shapes):
        b = torch.full((rows * cols + 16,), 3.0 if i == 3 else 0.0, dtype=TDT[dt], device=dev())
        sh = off[1] if off and off[0] == i else 0
        bufs.append(b)
        views.append(b[sh:sh + rows * cols].view(rows, cols))
    lse = torch.zeros(1, 1, S, device=dev())
    _reject(call_long(dt, views[0], None, views[1], views[2], lse, views[3], 1, S, 1, 0.0))
    torch.cuda.synchronize()
    assert (bufs[3] == 3).all(), "a rejected call wrote to dqkv"


@pytest.mark.parametrize("dt", DTS)
def test_long_backward_rejects_other_lengths(dt):
    for S in (128, 289):
        _rejected_call(dt, S)


@pytest.mark.parametrize("dt", ["x3", "pair"])
def test_long_backward_rejects_misaligned_pointers(dt):
    """x3: 4 bytes off, pair: 2 bytes off (one element each), for each of the four tensors in turn; nothing is written"""
    for which in range(4):
        _rejected_call(dt, 197, off=(which, 1))


def test_short_entry_still_rejects_16bit_above_128():
    """mmhip_op_attn_bwd keeps its dispatch: bf16 at S = 129 is rejected there"""
    S = 129
    qkv = torch.zeros(S, 192, dtype=torch.bfloat16, device=dev())
    ctx = torch.zeros(S, 64, dtype=torch.bfloat16, device=dev())
    lse = torch.zeros(1, 1, S, device=dev())
    dqkv = torch.full((S, 192), 3.0, dtype=torch.bfloat16, device=dev())
    _reject(rc_of("mmhip_op_attn_bwd", 0, ptr(qkv), None, ptr(ctx), ptr(ctx), ptr(lse), ptr(dqkv), 1, S, 1, 0.0, 0, 0, stream()))
    torch.cuda.synchronize()
    assert (dqkv == 3).all()
