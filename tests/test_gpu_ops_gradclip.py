"""-m gpu: global-norm gradient clipping at the operator level (include/mmhip.h mmhip_op_grad_clip, mmhip_adamw_clipped, mmhip_adamw_rows_clipped;
csrc/gradnorm.hip) against the fp64 reference and the derived bounds of tests/gradclip_ref.py (tests/test_gradclip_bounds_cpu.py shows that an fp32
computation in the kernels' order is inside them and six wrong variants are outside): all four public words, every buffer between sentinels, inputs
held to equality, every rejection with nothing written."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import adamw_ref as AR
import gpu_util as gu
import gradclip_ref as GR

pytestmark = pytest.mark.gpu

ALL = [(c, m) for c in GR.CASES for m in GR.MODES] + [("zeros", "zeros")]
GUARD = 64


def _bits(t):
    return t.view(torch.int32) if t.element_size() == 4 else t


def _state_block(fill=0):
    n = gu._lib.lib().mmhip_grad_clip_state_bytes()
    assert n == 16 + 4 * (GR.BLOCKS + GR.ROW_BLOCKS)
    return gu.guarded((n // 4,), torch.int32, fill)


def _words(view):
    w = view[:4].cpu()
    f = w.view(torch.float32)
    return float(f[1]), float(f[0]), int(w[2]), int(w[3])          # total, coef, clipped steps, steps


class _Call:
    """one mmhip_op_grad_clip call on guarded copies of a case's inputs"""

    def __init__(self, inp):
        self.inp = inp
        self.bufs = []
        for x in inp.segs:
            b = gu.guarded((len(x),), torch.float32, 0.0)
            b[1].copy_(torch.from_numpy(x))
            self.bufs.append((b[0], b[1], b[0].clone()))
        self.table = self.state = None
        self.rows, self.width = (0, 4) if inp.table is None else inp.table.shape
        if inp.table is not None:
            b = gu.guarded(tuple(inp.table.shape), torch.float32, 0.0)
            b[1].copy_(torch.from_numpy(inp.table))
            self.table = (b[0], b[1], b[0].clone())
            sb = torch.full((self.rows + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=gu.dev())
            sb[GUARD: GUARD + self.rows].copy_(torch.from_numpy(inp.state))
            self.state = (sb, sb[GUARD: GUARD + self.rows], sb.clone())
        k = max(len(inp.segs), 1)
        self.seg_g = (C.c_void_p * k)(*[b[1].data_ptr() for b in self.bufs])
        self.seg_n = (C.c_uint64 * k)(*[len(x) for x in inp.segs])

    def run(self, block, guard_words=None, max_norm=None, segments=None):
        return gu._lib.lib().mmhip_op_grad_clip(self.seg_g, self.seg_n, len(self.inp.segs) if segments is None else segments,
                                                gu.ptr(self.table[1]) if self.table else None, self.rows, self.width,
                                                gu.ptr(self.state[1]) if self.state else None, float(self.inp.max_norm) if max_norm is None else max_norm,
                                                float(self.inp.gs), gu.ptr(guard_words), gu.ptr(block), gu.stream())

    def inputs_untouched(self):
        every = self.bufs + [b for b in (self.table, self.state) if b is not None]
        return all(torch.equal(_bits(buf), _bits(snap)) for buf, _, snap in every)


@pytest.mark.parametrize("case,mode", ALL)
def test_grad_clip_against_float64(case, mode):
    inp = GR.build(case, mode)
    ref = GR.reference(inp)
    call = _Call(inp)
    buf, block, snap = _state_block()
    assert call.run(block) == 0
    torch.cuda.synchronize()
    total, coef, clipped, steps = _words(block)
    what = f"grad_clip {case} {mode}"
    print("margins grad_clip", case, mode, "k", ref.k, "total", round(abs(total - ref.total) / ref.b_total, 4) if ref.b_total else 0.0,
          "coef", round(abs(coef - ref.coef) / ref.b_coef, 4) if ref.b_coef else 0.0)
    assert gu.guards_intact(buf, snap, block.numel()), f"{what}: written outside the state block"
    assert call.inputs_untouched(), f"{what}: an input buffer or its sentinels changed"
    assert np.isfinite(total) and abs(total - ref.total) <= ref.b_total, f"{what}: total {total!r}, ref {ref.total!r}, bound {ref.b_total:.3e}"
    assert np.isfinite(coef) and abs(coef - ref.coef) <= ref.b_coef, f"{what}: coef {coef!r}, ref {ref.coef!r}, bound {ref.b_coef:.3e}"
    assert (clipped, steps) == (int(ref.clipped), 1), f"{what}: counters {(clipped, steps)}"
    if mode in ("under", "zeros"):
        assert np.float32(coef).view(np.uint32) == np.float32(1.0).view(np.uint32)


@pytest.mark.parametrize("case", ["3pass+1027", "dense+rows", "seg16"])
def test_same_call_twice_gives_the_same_bits(case):
    """the public words AND every partial sum: nothing in the order of summation is left to timing"""
    inp = GR.build(case, "half")
    call = _Call(inp)
    blocks = []
    for _ in range(2):
        _, block, _ = _state_block()
        assert call.run(block) == 0
        torch.cuda.synchronize()
        blocks.append(block.clone())
    assert torch.equal(blocks[0], blocks[1])
    used = (GR.BLOCKS if inp.segs else 0) + (GR.ROW_BLOCKS if inp.table is not None else 0)
    assert bool((blocks[0][4: 4 + used].view(torch.float32) >= 0).all()) and bool((blocks[0][4 + used:] == 0).all())


def test_counters_accumulate_and_a_void_step_leaves_them_alone():
    inp = GR.build("n1027", "half")
    call = _Call(inp)
    buf, block, snap = _state_block()
    guard = torch.tensor([7, 0], dtype=torch.int32, device=gu.dev())
    for want in ((1, 1), (2, 2)):
        assert call.run(block, guard) == 0
        torch.cuda.synchronize()
        assert _words(block)[2:] == want
    assert call.run(block, guard, max_norm=1e9) == 0                  # an unclipped step: only `steps` moves
    torch.cuda.synchronize()
    assert _words(block)[1:] == (1.0, 2, 3)
    guard[1] = 1                                                      # the step guard's flag: this step is void
    assert call.run(block, guard) == 0
    torch.cuda.synchronize()
    assert _words(block)[2:] == (2, 3) and guard.tolist() == [7, 1]
    assert gu.guards_intact(buf, snap, block.numel())


def _rejections():
    inp = GR.build("dense+rows", "half")
    call = _Call(inp)
    lib = gu._lib.lib()
    buf, block, snap = _state_block(0x5A5A5A5A)
    off = lambda t, nbytes: C.c_void_p(t.data_ptr() + nbytes)
    seg17 = GR.build("seg16", "half")
    big = _Call(GR.SimpleNamespace(segs=seg17.segs + [seg17.segs[0]], table=None, state=None, gs=seg17.gs, max_norm=seg17.max_norm))
    base = dict(seg_g=call.seg_g, seg_n=call.seg_n, segments=2, row_g=gu.ptr(call.table[1]), rows=call.rows, width=call.width, row_state=gu.ptr(call.state[1]),
                max_norm=1.0, grad_scale=1.0, guard=None, state=gu.ptr(block))
    null_seg = (C.c_void_p * 2)(call.bufs[0][1].data_ptr(), None)
    odd_seg = (C.c_void_p * 2)(call.bufs[0][1].data_ptr() + 4, call.bufs[1][1].data_ptr())
    guard = torch.zeros(4, dtype=torch.int32, device=gu.dev())
    bad = {"17 segments": dict(seg_g=big.seg_g, seg_n=big.seg_n, segments=17), "segments < 0": dict(segments=-1), "a null segment": dict(seg_g=null_seg),
           "a misaligned segment": dict(seg_g=odd_seg), "no segment arrays": dict(seg_g=None), "no state block": dict(state=None),
           "a misaligned state block": dict(state=off(block, 4)), "width % 4": dict(width=call.width + 2), "width 0": dict(width=0),
           "rows without row_state": dict(row_state=None), "rows without a table": dict(row_g=None), "a misaligned table": dict(row_g=off(call.table[1], 4)),
           "rows < 0": dict(rows=-1), "NaN max_norm": dict(max_norm=float("nan")), "inf max_norm": dict(max_norm=float("inf")),
           "max_norm 0": dict(max_norm=0.0), "max_norm < 0": dict(max_norm=-1.0), "NaN grad_scale": dict(grad_scale=float("nan")),
           "misaligned guard words": dict(guard=off(guard, 2))}
    for what, change in bad.items():
        a = dict(base, **change)
        rc = lib.mmhip_op_grad_clip(a["seg_g"], a["seg_n"], a["segments"], a["row_g"], a["rows"], a["width"], a["row_state"], a["max_norm"], a["grad_scale"],
                                    a["guard"], a["state"], gu.stream())
        yield what, rc
    torch.cuda.synchronize()
    yield "nothing written", 0 if (torch.equal(buf, snap) and call.inputs_untouched() and big.inputs_untouched()) else 1
    # the same arguments, unchanged, are accepted (the rejections above were the changes' doing)
    block.zero_()
    yield "the base call", lib.mmhip_op_grad_clip(*[base[k] for k in ("seg_g", "seg_n", "segments", "row_g", "rows", "width", "row_state", "max_norm", "grad_scale",
                                                                            "guard", "state")], gu.stream())
    torch.cuda.synchronize()


def test_bad_arguments_are_rejected_on_the_host_with_nothing_written():
    seen = dict(_rejections())
    assert seen.pop("nothing written") == 0 and seen.pop("the base call") == 0
    assert len(seen) == 19 and all(rc == -1 for rc in seen.values()), seen          # MMHIP_E_INVALID
    lib = gu._lib.lib()
    # the clipped AdamW forms reject a misaligned state block as well
    p, g, m, v = (torch.zeros(64, device=gu.dev()) for _ in range(4))
    _, block, _ = _state_block()
    odd = C.c_void_p(block.data_ptr() + 4)
    assert lib.mmhip_adamw_clipped(gu.ptr(p), gu.ptr(g), gu.ptr(m), gu.ptr(v), 64, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, 1, gu.stream(), None, odd) == -1
    st = torch.zeros(8, dtype=torch.uint8, device=gu.dev())
    assert lib.mmhip_adamw_rows_clipped(gu.ptr(p), gu.ptr(g), gu.ptr(m), gu.ptr(v), 8, 8, gu.ptr(st), 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, 1, gu.stream(), None,
                                        odd) == -1
    torch.cuda.synchronize()
    assert not bool(p.any()) and not bool(m.any())


# ---------------------------------------------------------------------------------------------------------------- AdamW with the coefficient
def _on_device(tensors):
    bufs = []
    for t in tensors:
        b = gu.guarded(tuple(t.shape), torch.float32, 0.0)
        b[1].copy_(t)
        bufs.append(b)
    return bufs


def _block_with_coef(coef):
    buf, block, _ = _state_block()
    block[:1].view(torch.float32).fill_(coef)
    return buf, block, buf.clone()


COMBOS = list(itertools.product(AR.STEPS, AR.GRAD_SCALES, (0, 1)))


@pytest.mark.parametrize("n", AR.NS)
def test_adamw_clipped(n):
    """state NULL: bit for bit mmhip_adamw_guarded.  With a state: p, m, v within tests/adamw_ref.py's bounds of the fp64 update on g * grad_scale * coef
    (grad_scale is 1 or 1/2 here, so the kernel's product grad_scale * coef is exact and the reference's rounding model is the kernel's)."""
    lr, wd, coef = 1e-3, 0.01, float(np.float32(0.37))
    state = AR.make_state(n)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for step, gs, zg in COMBOS:
        args = (n, lr, AR.BETA1, AR.BETA2, AR.EPS, wd, step, gs, zg, gu.stream(), None)
        a, b, c = _on_device(state), _on_device(state), _on_device(state)
        gu.call("mmhip_adamw_guarded", *[gu.ptr(x[1]) for x in a], *args)
        gu.call("mmhip_adamw_clipped", *[gu.ptr(x[1]) for x in b], *args, None)
        sbuf, block, ssnap = _block_with_coef(coef)
        gu.call("mmhip_adamw_clipped", *[gu.ptr(x[1]) for x in c], *args, gu.ptr(block))
        torch.cuda.synchronize()
        what = f"adamw_clipped n={n} step={step} gs={gs} zero_grad={zg}"
        for x, y in zip(a, b):
            assert torch.equal(x[0], y[0]), f"{what}: a null state is not the guarded form, bit for bit"
        assert torch.equal(sbuf, ssnap), f"{what}: the state block is read-only to AdamW"
        for name, (buf, view, snap) in zip("pgmv", c):
            assert gu.guards_intact(buf, snap, view.numel()), f"{what}: {name} written outside its buffer"
        h = AR.hyper(lr, wd, step, gs * coef)
        assert h.gs == float(np.float32(gs)) * coef
        ref, bound = AR.reference(*state, h)
        for name, got, r, bd in zip("pmv", (c[0][1], c[2][1], c[3][1]), ref, bound):
            worst[name] = max(worst[name], gu.assert_close_elementwise(got, r, bd, f"{what}: {name}"))
        assert torch.equal(c[1][1].cpu(), torch.zeros(n) if zg else state[1]), f"{what}: the gradient buffer is cleared or kept, never rescaled"
        # and the coefficient was really applied: the unclipped moments lie outside these bounds wherever the gradient is not negligible
        assert gu.violates_elementwise(a[2][1].cpu(), ref[1], bound[1]) > 0 or n == 1 and state[1][0] == 0
    print("margins adamw_clipped", n, {k: round(x, 4) for k, x in worst.items()})


@pytest.mark.parametrize("width", [8, 768])
def test_adamw_rows_clipped(width):
    lr, wd, coef = 1e-3, 0.01, float(np.float32(0.37))
    p0, g0, m0, v0, st0 = AR.rows_state(width)
    rows = len(AR.ROW_STATES)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for step, gs, zg in COMBOS:
        runs = []
        for form in ("guarded", "null", "state"):
            bufs = _on_device((p0, g0, m0, v0))
            st = st0.clone().to(gu.dev())
            sbuf, block, ssnap = _block_with_coef(coef)
            args = [gu.ptr(x[1]) for x in bufs] + [rows, width, gu.ptr(st), lr, AR.BETA1, AR.BETA2, AR.EPS, wd, step, gs, zg, gu.stream(), None]
            if form == "guarded":
                gu.call("mmhip_adamw_rows_guarded", *args)
            else:
                gu.call("mmhip_adamw_rows_clipped", *args, gu.ptr(block) if form == "state" else None)
            torch.cuda.synchronize()
            assert torch.equal(sbuf, ssnap)
            runs.append((bufs, st))
        what = f"adamw_rows_clipped width={width} step={step} gs={gs} zero_grad={zg}"
        for x, y in zip(runs[0][0], runs[1][0]):
            assert torch.equal(x[0], y[0]), f"{what}: a null state is not the guarded form, bit for bit"
        assert torch.equal(runs[0][1], runs[1][1])
        bufs, st = runs[2]
        h = AR.hyper(lr, wd, step, gs * coef)
        ref, bound, idle, exact_p, st_after, g_after = AR.rows_reference(p0, g0, m0, v0, st0, h, zg)
        for name, (buf, view, snap) in zip("pgmv", bufs):
            assert gu.guards_intact(buf, snap, view.numel()), f"{what}: {name} written outside its buffer"
        for name, got, r, bd in zip("pmv", (bufs[0][1], bufs[2][1], bufs[3][1]), ref, bound):
            live = ~idle
            worst[name] = max(worst[name], gu.assert_close_elementwise(got.cpu()[live], r[live], bd[live], f"{what}: {name}"))
        assert torch.equal(bufs[0][1].cpu()[idle], exact_p[idle]) and torch.equal(st.cpu(), st_after) and torch.equal(bufs[1][1].cpu(), g_after), what
    print("margins adamw_rows_clipped", width, {k: round(x, 4) for k, x in worst.items()})
