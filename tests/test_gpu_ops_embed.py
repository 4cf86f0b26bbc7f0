"""-m gpu: the text-embedding operators (include/mmhip.h mmhip_op_embed_fwd / mmhip_op_embed_bwd; csrc/rowops.hip pos_ids_kernel, embed_fwd_kernel,
embed_bwd_kernel, embed_scatter_det_kernel) against the fp64 references and the derived per-element bounds of tests/embed_ref.py
(tests/test_embed_bounds_cpu.py shows that an fp32 emulation of the kernels is inside them on these very cases and eight wrong variants are outside).
Every element of every output is compared; accumulated outputs are prefilled with non-zero values and rows nobody names must keep them to the bit;
every output sits between sentinels.  The backward is fed the reference forward's xhat (rounded to the activation type) and rstd (fp32): exactly
what the reference computes from, so the forward's rounding is not charged to it -- and both use one dropout mask, so a kept element's dx counts
and a dropped one's does not.  Cases: embed_ref.SHAPES x embed_ref.VARIANTS x {bf16, f16, x3}."""
import ctypes as C

import pytest
import torch

import embed_ref as ER
import gpu_util as gu
from op_bounds import pair_hi_is_nearest

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "f16", "x3"]
SHAPE_IDS = lambda s: "x".join(map(str, s))
_CASES = {}


def case(shape, k, dt):
    """the case, its forward reference (shared by the dtypes), and the dtype's bounds and backward reference: computed once, never modified"""
    if (shape, k) not in _CASES:
        c = ER.case_of(shape, k)
        _CASES[(shape, k)] = (c, ER.fwd_reference(c, c.p, c.seed), ER.keep_of(c, c.p, c.seed))
    c, fr, (keep, scale) = _CASES[(shape, k)]
    if (shape, k, dt) not in _CASES:
        bi = ER.bwd_inputs(c, fr, dt)
        _CASES[(shape, k, dt)] = (ER.fwd_bounds(c, fr, dt), bi) + ER.bwd_reference(c, bi, keep, scale, c.alpha)
    return (c, fr) + _CASES[(shape, k, dt)]


def _intact(out):
    for n, (buf, view, snap) in out.items():
        assert gu.guards_intact(buf, snap, view.numel()), f"{n}: written outside its buffer"


def _dev(t, dtype=None):
    return None if t is None else t.to(device=gu.dev(), dtype=dtype or t.dtype).contiguous()


def run_fwd(c, dt):
    code, tdt = gu.DT[dt]
    rows, H = c.rows, c.H
    out = {"x": gu.guarded((rows, H), tdt, float("nan")), "xhat": gu.guarded((rows, H), tdt, float("nan")), "rstd": gu.guarded((rows,), torch.float32, float("nan")),
           "pos_ids": gu.guarded((rows,), torch.int32, -7), "maskbias": gu.guarded((rows,), torch.float32, 7.0)}
    if dt == "x3":
        out["x_pair"] = gu.guarded((rows, 2 * H), torch.bfloat16, float("nan"))
    v = lambda n: out[n][1] if n in out else None
    ins = [_dev(t) for t in (c.ids, c.mask, c.type_ids, c.word, c.pos, c.type, c.gamma, c.beta)]
    gu.call("mmhip_op_embed_fwd", code, *[gu.ptr(t) for t in ins], ER.EPS, c.posts, c.T, H, c.xlmr, c.pad, c.p, c.seed, gu.ptr(v("x")), gu.ptr(v("xhat")),
            gu.ptr(v("rstd")), gu.ptr(v("pos_ids")), gu.ptr(v("maskbias")), gu.ptr(v("x_pair")), 2 * H, H, gu.stream())
    torch.cuda.synchronize()
    _intact(out)
    return {n: v(n).clone() for n in out}


ROW_STATE_GUARD = 64


def run_bwd(c, dt, bi, det=False, dx=None, p=None, partial=None, status_in=(0, 0)):
    """the backward on prefilled outputs; returns the outputs, row_state (whole buffer, with its margins) and its prefill, the status words"""
    code, tdt = gu.DT[dt]
    rows, H = c.rows, c.H
    p = c.p if p is None else p
    partial = c.partial if partial is None else partial
    out = {}
    for n, pre in c.pre.items():
        out[n] = gu.guarded(tuple(pre.shape), torch.float32, 0.0)
        out[n][1].copy_(pre)
    type_rows = 2 if c.tt == "two" else 0
    nbytes = gu._lib.lib().mmhip_op_embed_bwd_ws_bytes(c.posts, c.T, H, type_rows)
    nblk = c.T * ((c.posts + 15) // 16)
    assert nbytes == (4 if type_rows == 2 else 3) * nblk * H * 4
    if partial:
        out["partial"] = gu.guarded((nbytes // 4,), torch.float32, float("nan"))
    if det:
        out["det_rows"] = gu.guarded((rows, H), torch.float32, float("nan"))
    v = lambda n: out[n][1] if n in out else None
    g = torch.Generator().manual_seed(5)
    n4 = (c.vocab + 3) // 4 * 4                                  # the flags live in 32-bit words: the array is rounded up to four bytes
    rs_pre = (torch.randint(0, 256, (n4 + 2 * ROW_STATE_GUARD,), generator=g) & 0xFE).to(torch.uint8)
    rs = _dev(rs_pre)
    status = torch.tensor(status_in, dtype=torch.int32, device=gu.dev())
    ins = [_dev((bi.dx if dx is None else dx), tdt), _dev(bi.xhat, tdt), _dev(bi.rstd, torch.float32), _dev(c.gamma), _dev(c.ids), _dev(bi.pos_ids, torch.int32),
           _dev(c.type_ids)]
    gu.call("mmhip_op_embed_bwd", code, *[gu.ptr(t) for t in ins], type_rows, c.posts, c.T, H, c.pad, c.pos_pad, p, c.seed, c.alpha, gu.ptr(v("dword")),
            gu.ptr(v("dpos")), gu.ptr(v("dtype")), gu.ptr(v("dgamma")), gu.ptr(v("dbeta")), gu.ptr(v("partial")), nbytes if partial else 0,
            C.c_void_p(rs.data_ptr() + ROW_STATE_GUARD), gu.ptr(v("det_rows")), c.max_pos if det else 0, gu.ptr(status), gu.stream())
    torch.cuda.synchronize()
    _intact(out)
    return {n: v(n).clone() for n in out}, rs.cpu(), rs_pre, status.cpu()


def check_row_state(c, rs, rs_pre):
    G = ROW_STATE_GUARD
    assert torch.equal(rs[:G], rs_pre[:G]) and torch.equal(rs[G + c.vocab:], rs_pre[G + c.vocab:]), "row_state: bytes outside the table changed"
    assert torch.equal(rs[G:G + c.vocab], ER.row_state_reference(c, rs_pre[G:G + c.vocab])), "row_state: bit 0 is not exactly the ids that occur"


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", range(len(ER.VARIANTS)))
@pytest.mark.parametrize("shape", ER.SHAPES, ids=SHAPE_IDS)
def test_embed_forward_against_float64(shape, k, dt):
    c, fr, fb, *_ = case(shape, k, dt)
    got = run_fwd(c, dt)
    z = torch.zeros(c.rows, dtype=torch.float64)
    gu.assert_close_elementwise(got["pos_ids"], fr.pos_ids.double(), z, f"pos_ids {shape} {k}")
    assert torch.equal(got["maskbias"].double().cpu(), fr.maskbias), "maskbias"
    m = {n: gu.assert_close_elementwise(got[n], getattr(fr, n), fb[n], f"embed fwd {n} {shape} {k} {dt}") for n in ("x", "xhat", "rstd")}
    assert bool((got["x"].double().cpu()[fr.ks == 0] == 0).all())
    if dt == "x3":
        pair = got["x_pair"].cpu()
        hi, lo = pair[:, :c.H], pair[:, c.H:]
        m["x_pair"] = gu.assert_close_elementwise(hi.double() + lo.double(), fr.x, fb["x_pair"], f"embed fwd x_pair {shape} {k}")
        assert pair_hi_is_nearest(hi, lo).all()
    print("margins embed_fwd", dt, shape, k, {a: round(b, 4) for a, b in m.items()})


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", range(len(ER.VARIANTS)))
@pytest.mark.parametrize("shape", ER.SHAPES, ids=SHAPE_IDS)
def test_embed_backward_against_float64(shape, k, dt):
    c, fr, fb, bi, ref, b = case(shape, k, dt)
    got, rs, rs_pre, status = run_bwd(c, dt, bi)
    m = {n: gu.assert_close_elementwise(got[n], ref[n], b[n], f"embed bwd {n} {shape} {k} {dt}") for n in ("dword", "dpos", "dtype", "dgamma", "dbeta")}
    check_row_state(c, rs, rs_pre)
    assert status.tolist() == [0, 0], "all-finite dx: the guard words stay 0"
    print("margins embed_bwd", dt, shape, k, {a: round(b_, 4) for a, b_ in m.items()})


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("k", [2, 3, 7])
@pytest.mark.parametrize("shape", [(5, 3, 132), (17, 65, 768), (33, 130, 256)], ids=SHAPE_IDS)
def test_embed_backward_deterministic_scatter(shape, k, dt):
    """det_rows given: per-slot rows within their bound, dword / dpos within the same bounds as the atomic path, and the same bits on a second call"""
    c, fr, fb, bi, ref, b = case(shape, k, dt)
    a, rs, rs_pre, _ = run_bwd(c, dt, bi, det=True)
    a2, *_ = run_bwd(c, dt, bi, det=True)
    m = {n: gu.assert_close_elementwise(a[n], ref[n], b[n], f"embed bwd det {n} {shape} {k} {dt}") for n in ("det_rows", "dword", "dpos", "dtype", "dgamma", "dbeta")}
    check_row_state(c, rs, rs_pre)
    for n in ("dword", "dpos", "det_rows"):
        assert torch.equal(a[n].view(torch.int32), a2[n].view(torch.int32)), n
    print("margins embed_bwd_det", dt, shape, k, {a_: round(b_, 4) for a_, b_ in m.items()})


@pytest.mark.parametrize("dt", DTYPES)
def test_embed_backward_counts_one_wave_for_one_inf(dt):
    """a single inf in one row of dx (no dropout: the element is read): the flag word is 1 and the counter is the number of waves that saw it, 1;
    the words are added to / OR-ed, not stored.  Non-finite data is ordinary input here: the call returns and stays inside its buffers."""
    shape, k = (5, 3, 132), 1
    c, fr, fb, bi, ref, b = case(shape, k, dt)
    assert c.p == 0
    dx = bi.dx.clone()
    dx[2 * c.T + 1, 17] = float("inf")
    _, _, _, status = run_bwd(c, dt, bi, dx=dx, status_in=(4, 2))
    assert status.tolist() == [5, 3]
    _, _, _, status = run_bwd(c, dt, bi, dx=dx)
    assert status.tolist() == [1, 1]


def _fwd_args(**kw):
    """a valid small call on real buffers (posts 2, T 3, H 8), fields overridable; every output filled with 7"""
    dev = gu.dev()
    posts, T, H = 2, 3, 8
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    s7 = lambda *s, dt=torch.float32: torch.full(s, 7, dtype=dt, device=dev)
    t = dict(ids=z(6, dt=torch.int64), mask=z(6, dt=torch.int64), type_ids=None, word=z(4, 16), pos=z(8, 16), type=z(2, 16), gamma=z(16), beta=z(16),
             x=s7(6, 16), xhat=s7(6, 16), rstd=s7(6), pos_ids=s7(6, dt=torch.int32), maskbias=s7(6), x_pair=None)
    a = dict(dtype=2, eps=1e-5, posts=posts, T=T, H=H, xlmr=1, pad_id=1, p=0.0, seed=1, ld_pair=2 * H, lo_pair=H)
    off = kw.pop("offset", {})
    a.update(kw)
    t.update({n: a.pop(n) for n in list(a) if n in t})
    P = lambda n: None if t[n] is None else C.c_void_p(t[n].data_ptr() + off.get(n, 0))
    args = [a["dtype"], P("ids"), P("mask"), P("type_ids"), P("word"), P("pos"), P("type"), P("gamma"), P("beta"), a["eps"], a["posts"], a["T"], a["H"], a["xlmr"],
            a["pad_id"], a["p"], a["seed"], P("x"), P("xhat"), P("rstd"), P("pos_ids"), P("maskbias"), P("x_pair"), a["ld_pair"], a["lo_pair"], gu.stream()]
    return args, [t[n] for n in ("x", "xhat", "rstd", "pos_ids", "maskbias")]


def _bwd_args(**kw):
    dev = gu.dev()
    posts, T, H = 2, 3, 8
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    s7 = lambda *s, dt=torch.float32: torch.full(s, 7, dtype=dt, device=dev)
    t = dict(dx=z(6, 16), xhat=z(6, 16), rstd=z(6), gamma=z(16), ids=z(6, dt=torch.int64), pos_ids=z(6, dt=torch.int32), type_ids=None, dword=s7(4, 16),
             dpos=s7(8, 16), dtype_rows=s7(2, 16), dgamma=s7(16), dbeta=s7(16), partial=None, row_state=None, det_rows=None, status=None)
    a = dict(dtype=2, type_rows=0, posts=posts, T=T, H=H, pad_id=1, pos_pad_id=1, p=0.0, seed=1, alpha=1.0, partial_bytes=0, max_pos=0)
    off = kw.pop("offset", {})
    a.update(kw)
    t.update({n: a.pop(n) for n in list(a) if n in t})
    P = lambda n: None if t[n] is None else C.c_void_p(t[n].data_ptr() + off.get(n, 0))
    args = [a["dtype"], P("dx"), P("xhat"), P("rstd"), P("gamma"), P("ids"), P("pos_ids"), P("type_ids"), a["type_rows"], a["posts"], a["T"], a["H"], a["pad_id"],
            a["pos_pad_id"], a["p"], a["seed"], a["alpha"], P("dword"), P("dpos"), P("dtype_rows"), P("dgamma"), P("dbeta"), P("partial"), a["partial_bytes"],
            P("row_state"), P("det_rows"), a["max_pos"], P("status"), gu.stream()]
    outs = [t[n] for n in ("dword", "dpos", "dtype_rows", "dgamma", "dbeta")] + [t[n] for n in ("partial", "det_rows") if t[n] is not None]
    return args, outs


FWD_REJECTS = [dict(ids=None), dict(mask=None), dict(word=None), dict(gamma=None), dict(x=None), dict(pos_ids=None), dict(maskbias=None), dict(posts=0), dict(T=0),
               dict(H=0), dict(H=6), dict(H=1028), dict(p=-0.1), dict(p=1.0), dict(dtype=3), dict(offset=dict(word=4)), dict(offset=dict(beta=8)),
               dict(offset=dict(x=8)), dict(offset=dict(xhat=4)), dict(dtype=0, x_pair="x"), dict(x_pair="x", lo_pair=4), dict(x_pair="x", offset=dict(x_pair=8))]
BWD_REJECTS = [(dict(dx=None), -1), (dict(rstd=None), -1), (dict(pos_ids=None), -1), (dict(dword=None), -1), (dict(dbeta=None), -1), (dict(posts=0), -1),
               (dict(T=-1), -1), (dict(H=6), -1), (dict(H=1028), -1), (dict(p=1.0), -1), (dict(p=float("nan")), -1), (dict(dtype=3), -1), (dict(type_rows=2), -1),
               (dict(det_rows="d", max_pos=0), -1), (dict(offset=dict(dx=8)), -1), (dict(offset=dict(gamma=4)), -1), (dict(det_rows="d", max_pos=8, offset=dict(det_rows=4)), -1),
               (dict(row_state="r", offset=dict(row_state=1)), -1), (dict(partial="p", partial_bytes=3 * 3 * 8 * 4 - 4), -3),
               (dict(partial="p", partial_bytes=3 * 3 * 8 * 4, type_rows=2, type_ids="t"), -3)]


@pytest.mark.parametrize("bad", FWD_REJECTS, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()).replace(" ", ""))
def test_embed_forward_rejects_on_the_host(bad):
    bad = dict(bad)
    if bad.get("x_pair") == "x":
        bad["x_pair"] = torch.full((6, 32), 7, dtype=torch.bfloat16, device=gu.dev())
    args, outs = _fwd_args(**bad)
    assert gu._lib.lib().mmhip_op_embed_fwd(*args) == -1
    torch.cuda.synchronize()
    for t in outs + ([bad["x_pair"]] if bad.get("x_pair") is not None else []):
        assert t is None or bool((t == 7).all())


@pytest.mark.parametrize("bad,rc", BWD_REJECTS, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()).replace(" ", "") if isinstance(b, dict) else str(b))
def test_embed_backward_rejects_on_the_host(bad, rc):
    bad = dict(bad)
    dev = gu.dev()
    fills = {"d": lambda: torch.full((6, 16), 7.0, device=dev), "r": lambda: torch.full((8,), 7, dtype=torch.uint8, device=dev),
             "p": lambda: torch.full((4 * 3 * 8,), 7.0, device=dev), "t": lambda: torch.zeros(6, dtype=torch.int64, device=dev)}
    for n in ("det_rows", "row_state", "partial", "type_ids"):
        if isinstance(bad.get(n), str):
            bad[n] = fills[bad[n]]()
    args, outs = _bwd_args(**bad)
    assert gu._lib.lib().mmhip_op_embed_bwd(*args) == rc
    torch.cuda.synchronize()
    for t in outs + ([bad["row_state"]] if bad.get("row_state") is not None else []):
        assert t is None or bool((t == 7).all())
    assert gu._lib.lib().mmhip_op_embed_bwd(*_bwd_args()[0]) == 0          # the unmodified call is a valid one
