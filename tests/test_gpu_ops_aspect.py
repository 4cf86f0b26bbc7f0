"""-m gpu: the aspect-att fusion operator pair (include/mmhip.h mmhip_op_aspect_fusion_fwd / _bwd; csrc/heads.hip) against the float64 reference of
tests/aspect_ref.py, element by element, within bounds derived there from fp32 unit roundoff, the kernel's dot depth, the magnitude sums and the
documented error of tanhf / expf.  Shapes: one post; two posts (text with text, image with image); an odd batch (a mixed post); one full
workgroup of eight posts; 65 posts -- nine workgroups, the last with one post, d a / d b summed over nine partial rows.  Inputs are scaled so
that pre-tanh values reach about +-2.  The measured worst ratios are in profiles/op_test_margins.md."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aspect_ref as R

if torch.cuda.is_available():
    import smtc_amd  # noqa: F401
    from smtc_amd import _lib
    from gpu_util import assert_close_elementwise, call, dev, guarded, guards_intact, ptr, stream

SHAPES = [(1, 128), (2, 128), (3, 768), (8, 768), (65, 768)]
SENTINEL = 7.25


def inputs(B, H):
    g = torch.Generator().manual_seed(1000 * B + H)
    t_pool, v_pool = (torch.tanh(torch.randn(B, H, generator=g)) for _ in range(2))          # pooler outputs lie in (-1, 1)
    a = torch.randn(H, generator=g) * (2.0 / (0.63 * H ** 0.5))          # std of V . a about 2 (|tanh(N(0, 1))| has rms 0.63) ...
    b = torch.randn(1, generator=g) * 0.1
    d_feats = torch.randn(B, H, generator=g)
    d_t0 = torch.randn(B, H, generator=g)
    return t_pool, v_pool, a, b, d_feats, d_t0


def run(B, H, accumulate, x=None):
    """-> dict of the guarded outputs (views, on the device) after one forward + backward; asserts the guard bands"""
    t_pool, v_pool, a, b, d_feats, d_t0 = x or inputs(B, H)
    D = lambda t: t.to(dev()).contiguous()
    tp, vp, aa, bb, df = D(t_pool), D(v_pool), D(a), D(b), D(d_feats)
    bufs = {k: guarded(shape, torch.float32, SENTINEL) for k, shape in
            dict(feats=(B, H), w=(B, 2), e=(B, 2), d_tpool=(B, H), da=(H,), db=(1,)).items()}
    v = {k: x[1] for k, x in bufs.items()}
    if accumulate:
        v["d_tpool"].copy_(d_t0)
        v["da"].fill_(1.5)
        v["db"].fill_(-0.5)
    ws_bytes = int(_lib.lib().mmhip_op_aspect_fusion_ws_bytes(B, H))
    ws_buf, ws, ws_snap = guarded((ws_bytes // 4,), torch.float32, 0.0)
    call("mmhip_op_aspect_fusion_fwd", ptr(tp), ptr(vp), ptr(aa), ptr(bb), B, H, ptr(v["feats"]), ptr(v["w"]), ptr(v["e"]), stream())
    call("mmhip_op_aspect_fusion_bwd", ptr(tp), ptr(vp), ptr(aa), ptr(bb), B, H, ptr(v["feats"]), ptr(v["w"]), ptr(v["e"]), ptr(df), ptr(v["d_tpool"]),
         ptr(v["da"]), ptr(v["db"]), int(accumulate), int(accumulate), ptr(ws), ws_bytes, stream())
    torch.cuda.synchronize()
    for k, (buf, view, snap) in bufs.items():
        assert guards_intact(buf, snap, view.numel()), k
    assert guards_intact(ws_buf, ws_snap, ws.numel())
    # (the operator has no output for the image rows at all -- the tower is frozen; that row B and beyond are not written shows in d_tpool's guard band)
    return v


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("B,H", SHAPES)
def test_forward_and_backward_within_derived_bounds(B, H, accumulate):
    x = inputs(B, H)
    t_pool, v_pool, a, b, d_feats, d_t0 = x
    v = run(B, H, accumulate, x)
    feats = v["feats"].cpu().numpy()
    r = R.op_reference(t_pool.numpy(), v_pool.numpy(), a.numpy(), b.numpy(), d_feats.numpy(), d_t0.numpy() if accumulate else None, relu_mask=feats > 0)
    bd = R.op_bounds(r, a.numpy(), d_feats.numpy(), d_t0.numpy() if accumulate else None)
    assert np.abs(r["pre"]).max() > 1.0 and np.abs(r["w"][:, 0] - 0.5).max() > 0.1 and 0.25 < (r["mix"] > 0).mean() < 0.75
    # the kernel's ReLU pattern may differ from the reference's only where |mix| is within the forward bound
    assert not ((feats > 0) != (r["mix"] > 0))[~bd["relu_unsafe"]].any()
    T = lambda k: torch.from_numpy(np.asarray(r[k], dtype=np.float64))
    Bd = lambda k: torch.from_numpy(np.asarray(bd[k], dtype=np.float64))
    margins = {k: assert_close_elementwise(v[k], T(k), Bd(k), f"{k} B={B} H={H}") for k in ("feats", "w", "e", "d_tpool")}
    off = 1.5 if accumulate else 0.0          # the preset d a; its addition is one more rounding
    margins["da"] = assert_close_elementwise(v["da"], T("da") + off, Bd("da") + R.U * (T("da") + off).abs(), f"da B={B} H={H}")
    offb = -0.5 if accumulate else 0.0
    margins["db"] = assert_close_elementwise(v["db"], (T("db") + offb).reshape(1), (Bd("db") + R.U * (T("db") + offb).abs()).reshape(1), f"db B={B}")
    print("ASPECT_MARGIN", B, H, accumulate, {k: float("%.3g" % m) for k, m in margins.items()})
    # softmax weights of a post sum to one
    assert (v["w"].sum(dim=1) - 1).abs().max().item() <= 4 * R.U * 2


@pytest.mark.parametrize("B,H", [(3, 768), (65, 768)])
def test_two_calls_give_equal_bits(B, H):
    x = inputs(B, H)
    one, two = run(B, H, 1, x), run(B, H, 1, x)
    for k in ("feats", "w", "e", "d_tpool", "da", "db"):
        assert torch.equal(one[k].view(torch.int32), two[k].view(torch.int32)), k


def test_host_side_rejects():
    lib = _lib.lib()
    z = torch.zeros(4 * 1024 + 64, device=dev())
    p = ptr(z)
    for B, H in ((0, 128), (1, 96), (1, 32), (1, 1088)):
        assert lib.mmhip_op_aspect_fusion_fwd(p, p, p, p, B, H, p, p, p, stream()) == -1
        assert lib.mmhip_op_aspect_fusion_bwd(p, p, p, p, B, H, p, p, p, p, p, p, p, 0, 0, p, 1 << 20, stream()) == -1
    assert lib.mmhip_op_aspect_fusion_fwd(None, p, p, p, 1, 128, p, p, p, stream()) == -1
    assert lib.mmhip_op_aspect_fusion_bwd(p, p, p, p, 2, 128, p, p, p, p, p, p, p, 0, 0, p, 16, stream()) == -3          # scratch too small
    assert lib.mmhip_op_aspect_fusion_ws_bytes(65, 768) == 9 * (768 + 4) * 4
    torch.cuda.synchronize()
    assert z.abs().max().item() == 0.0          # nothing was written
