"""No GPU: mmhip_op_attn_bwd_long (the attention backward for 129..288 keys) is declared, exported and rejects what it does not take on the host
side, before any GPU work; and the bounds tests/test_gpu_ops_attention_long_bwd.py holds it to mean something at ITS sizes and masks -- a CPU
emulation of the kernel's roundings stays inside op_bounds.attn_bwd_bounds, an off-by-one attention (one key dropped, the score scale off by 2^-6, the
next dropout stream) leaves them on dq, dk and dv."""
import ctypes as C
import os
import re

import pytest

import op_bounds as OB
import attn_long_cases as AL
from gpu_util import assert_close_elementwise, violates_elementwise
from smtc_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mmhip_op_attn_bwd_long"


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def test_declared_and_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "mmhip.h")).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr)
    assert NAME in _lib.EXPORTS and hasattr(lib, NAME)
    assert _lib._SIGS[NAME] == _lib._SIGS["mmhip_op_attn_bwd"]          # same signature, same dtype codes


def test_rejects_on_the_host_side(lib):
    """dummy (never dereferenced) pointers: every one of these returns MMHIP_E_INVALID before any HIP call"""
    fn = getattr(lib, NAME)
    buf = C.create_string_buffer(256)
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)                       # 16-byte aligned, non-null

    def rc(dtype=0, S=197, posts=1, heads=1, qkv=p, ctx=p, dctx=p, lse=p, dqkv=p):
        return fn(dtype, qkv, None, ctx, dctx, lse, dqkv, posts, S, heads, 0.0, 0, 0, None)

    for S in (0, 128, 289):
        for dtype in (0, 1, 2, 3):
            assert rc(dtype=dtype, S=S) == -1, (dtype, S)
    assert rc(heads=0) == -1 and rc(posts=0) == -1 and rc(dtype=7) == -1 and rc(dtype=-1) == -1
    for name in ("qkv", "ctx", "dctx", "lse", "dqkv"):
        assert rc(**{name: None}) == -1, name
    off = C.c_void_p(p.value + 4)
    for name in ("qkv", "ctx", "dctx", "dqkv"):
        for dtype in (2, 3):
            assert rc(dtype=dtype, **{name: off}) == -1, (name, dtype)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [197, 288])
@pytest.mark.parametrize("dt", ["bf16", "f16", "x3", "pair"])
def test_bounds_hold_the_emulation_and_see_an_off_by_one(dt, S, p):
    posts, heads = 5, 2
    r = AL.case(dt, posts, S, heads, p).r
    bounds = OB.attn_bwd_bounds(r, dt, S)
    _, _, dq, dk, dv = OB.attn_emulate(r, dt)
    ms = [assert_close_elementwise(got, ref, b, "emulated " + name)
          for name, got, ref, b in zip(("dq", "dk", "dv"), (dq, dk, dv), (r.dq, r.dk, r.dv), bounds)]
    dead = ~r.live[:, :, 0, :]
    assert dead.any() and (bounds[1][dead] == 0).all() and (bounds[2][dead] == 0).all()
    wrong = {"key dropped": AL.reference(dt, posts, S, heads, p, drop_last_key_of=(0, 1)).r,
             "score scale": AL.reference(dt, posts, S, heads, p, score_scale=0.125 * (1 + 2.0 ** -6)).r}
    if p:
        wrong["dropout stream"] = AL.reference(dt, posts, S, heads, p, sid=17).r
    out = []
    for what, w in wrong.items():
        for name, got, ref, b in zip(("dq", "dk", "dv"), (w.dq, w.dk, w.dv), (r.dq, r.dk, r.dv), bounds):
            n = violates_elementwise(got, ref, b)
            out.append(n)
            assert n > 0, (what, name)
    print(f"MARGIN attn_bwd_long_bounds {dt} S={S} p={p} emulation dq={ms[0]:.4f} dk={ms[1]:.4f} dv={ms[2]:.4f} fewest elements outside={min(out)}")
