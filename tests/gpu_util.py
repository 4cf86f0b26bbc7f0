"""helpers for the -m gpu tests: device buffers via torch, calls through the C ABI (ctypes)."""
import ctypes as C

import numpy as np
import torch

import smtc_amd  # noqa: F401
from smtc_amd import _lib

DT = {"bf16": (_lib.BF16, torch.bfloat16), "f16": (_lib.F16, torch.float16), "x3": (_lib.F32, torch.float32)}


def dev():
    return torch.device("cuda:0")


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name, *args):
    rc = getattr(_lib.lib(), name)(*args)
    assert rc == 0, f"{name} returned {rc}"


def rel_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def assert_close_elementwise(got, ref, bound, what):
    """|got - ref| <= bound for EVERY element (ref, bound: fp64 CPU tensors of one shape; got: anything .double().cpu() takes).  Returns the margin
    max(|got - ref| / bound); where bound == 0 the element must match exactly.  A NaN / inf in `got` fails.  rel_err above divides by the tensor's
    largest magnitude and so cannot see an error confined to small elements; this can."""
    got = got.detach().double().cpu().reshape(ref.shape)
    ref, bound = ref.detach().double(), bound.detach().double()
    assert ref.shape == bound.shape and (bound >= 0).all(), what
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    worst = ratio.max().item() if ratio.numel() else 0.0
    if not worst <= 1.0:
        idx = np.unravel_index(int(torch.argmax(ratio.flatten())), tuple(ref.shape))
        raise AssertionError(f"{what}: worst element {tuple(int(i) for i in idx)}: got {got[idx].item()!r}, ref {ref[idx].item()!r}, "
                             f"|err| {err[idx].item():.3e}, bound {bound[idx].item():.3e}, ratio {worst:.3g}; "
                             f"{int((ratio > 1).sum())} of {ratio.numel()} elements outside")
    return worst


def violates_elementwise(got, ref, bound):
    """number of elements with |got - ref| > bound (the sensitivity checks: a subtly wrong result must leave the bound somewhere)"""
    return int(((got.double() - ref.double()).abs() > bound.double()).sum())


def guarded(shape, dtype, fill, guard=64, device=None):
    """a tensor of `shape` inside one allocation with `guard` sentinel elements on either side: (whole buffer, view, sentinel snapshot).  An
    overrun of a kernel lands in the test's own buffer; guards_intact() reports it."""
    n = int(np.prod(shape))
    buf = torch.empty(n + 2 * guard, dtype=dtype, device=device or dev())
    buf.view(torch.int16 if buf.element_size() == 2 else torch.int32).fill_(0x5A5A if buf.element_size() == 2 else 0x5A5A5A5A)
    view = buf[guard:guard + n].view(*shape)
    view.fill_(fill)
    return buf, view, buf.clone()


def guards_intact(buf, snapshot, n, guard=64):
    it = torch.int16 if buf.element_size() == 2 else torch.int32
    a, b = buf.view(it), snapshot.view(it)
    return bool(torch.equal(a[:guard], b[:guard]) and torch.equal(a[guard + n:], b[guard + n:]))


def keep_mask(shape, stream_id, seed, p, offset=0):
    """the kernels' dropout keep mask for a row-major tensor of `shape` (oracle/mm_oracle.py hash)"""
    from oracle import mm_oracle as O
    n = int(np.prod(shape))
    return torch.from_numpy(O.hash_keep_mask(n, offset, stream_id, seed, p)).view(*shape), O.keep_scale(p)
