"""-m gpu: the fused AdamW (include/mmhip.h mmhip_adamw / mmhip_adamw_rows; csrc/heads.hip adamw_kernel, adamw_rows_kernel) against the fp64 reference
and the derived per-element bounds of tests/adamw_ref.py (tests/test_adamw_bounds_cpu.py shows that an fp32 computation is inside them and four wrong
variants are outside): every element of p, m and v, all four buffers between sentinels, the gradient buffer and the row state bytes held to equality."""
import itertools

import pytest
import torch

import adamw_ref as AR
import gpu_util as gu

pytestmark = pytest.mark.gpu

COMBOS = list(itertools.product(AR.STEPS, AR.GRAD_SCALES, (0, 1)))


def _on_device(tensors):
    bufs = []
    for t in tensors:
        b = gu.guarded(tuple(t.shape), torch.float32, 0.0)
        b[1].copy_(t)
        bufs.append(b)
    return bufs


def _guards(bufs, what):
    for name, (buf, view, snap) in zip("pgmv", bufs):
        assert gu.guards_intact(buf, snap, view.numel()), f"{what}: {name} written outside its buffer"


@pytest.mark.parametrize("lr,wd", AR.LR_WD)
@pytest.mark.parametrize("n", AR.NS)
def test_adamw_against_float64(n, lr, wd):
    state = AR.make_state(n)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for step, gs, zg in COMBOS:
        h = AR.hyper(lr, wd, step, gs)
        ref, bound = AR.reference(*state, h)
        bufs = _on_device(state)
        p, g, m, v = (b[1] for b in bufs)
        gu.call("mmhip_adamw", gu.ptr(p), gu.ptr(g), gu.ptr(m), gu.ptr(v), n, lr, AR.BETA1, AR.BETA2, AR.EPS, wd, step, gs, zg, gu.stream())
        torch.cuda.synchronize()
        what = f"adamw n={n} lr={lr} wd={wd} step={step} gs={gs} zero_grad={zg}"
        _guards(bufs, what)
        for name, got, r, b in zip("pmv", (p, m, v), ref, bound):
            worst[name] = max(worst[name], gu.assert_close_elementwise(got, r, b, f"{what}: {name}"))
        assert torch.equal(g.cpu(), torch.zeros(n) if zg else state[1]), f"{what}: the gradient buffer"
    print("margins adamw", (n, lr, wd), {k: round(x, 4) for k, x in worst.items()})


@pytest.mark.parametrize("lr,wd", AR.LR_WD)
@pytest.mark.parametrize("width", AR.ROW_WIDTHS)
def test_adamw_rows_against_float64(width, lr, wd):
    p0, g0, m0, v0, st0 = AR.rows_state(width)
    rows = len(AR.ROW_STATES)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for step, gs, zg in COMBOS:
        h = AR.hyper(lr, wd, step, gs)
        ref, bound, idle, exact_p, st_after, g_after = AR.rows_reference(p0, g0, m0, v0, st0, h, zg)
        bufs = _on_device((p0, g0, m0, v0))
        p, g, m, v = (b[1] for b in bufs)
        sbuf, st, ssnap = gu.guarded((rows,), torch.int16, 0, guard=64)          # bytes inside 16-bit sentinels: 2 * rows bytes, the first `rows` are the states
        stb = st.view(torch.uint8)
        stb.fill_(0x5A)
        stb[:rows].copy_(st0)
        gu.call("mmhip_adamw_rows", gu.ptr(p), gu.ptr(g), gu.ptr(m), gu.ptr(v), rows, width, gu.ptr(stb), lr, AR.BETA1, AR.BETA2, AR.EPS, wd, step, gs, zg,
                gu.stream())
        torch.cuda.synchronize()
        what = f"adamw_rows width={width} lr={lr} wd={wd} step={step} gs={gs} zero_grad={zg}"
        _guards(bufs, what)
        assert gu.guards_intact(sbuf, ssnap, rows), f"{what}: row state written outside its buffer"
        assert torch.equal(stb[:rows].cpu(), st_after) and bool((stb[rows:] == 0x5A).all()), f"{what}: state bytes {stb[:rows].tolist()}"
        for name, got, r, b in zip("pmv", (p, m, v), ref, bound):
            worst[name] = max(worst[name], gu.assert_close_elementwise(got, r, b, f"{what}: {name}"))
        assert torch.equal(p.cpu()[idle], exact_p[idle]), f"{what}: decay-only rows are p * (1 - lr wd) in fp32, bit for bit"
        assert torch.equal(m.cpu()[idle], m0[idle]) and torch.equal(v.cpu()[idle], v0[idle]), f"{what}: moments of decay-only rows"
        assert torch.equal(g.cpu(), g_after), f"{what}: the gradient buffer"
    print("margins adamw_rows", (width, lr, wd), {k: round(x, 4) for k, x in worst.items()})


def test_adamw_second_pass_of_the_grid_stride_loop():
    """n = 16384 * 1024 + 1024 + 3: the first 256 four-vectors' workgroup comes round a second time, and three elements are left for the tail"""
    n, dev = AR.BIG_N, gu.dev()
    lr, wd, step, gs = 1e-3, 0.01, 2, 0.5
    h = AR.hyper(lr, wd, step, gs)
    state = AR.make_state_on(n, dev)
    ref, bound = AR.reference(*state, h)
    bufs = _on_device(state)
    del state
    p, g, m, v = (b[1] for b in bufs)
    gu.call("mmhip_adamw", gu.ptr(p), gu.ptr(g), gu.ptr(m), gu.ptr(v), n, lr, AR.BETA1, AR.BETA2, AR.EPS, wd, step, gs, 1, gu.stream())
    torch.cuda.synchronize()
    _guards(bufs, "adamw big")
    worst = {}
    for name, got, r, b in zip("pmv", (p, m, v), ref, bound):
        err = (got.double() - r).abs()
        err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
        ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        worst[name] = ratio.max().item()
        del err, ratio
        if not worst[name] <= 1.0:
            gu.assert_close_elementwise(got, r.cpu(), b.cpu(), f"adamw big: {name}")
    assert not bool(g.any()), "adamw big: the gradient buffer is cleared"
    print("margins adamw big", n, {k: round(x, 4) for k, x in worst.items()})


def test_adamw_counts_a_nonfinite_gradient_in_the_tail():
    """the only non-finite element lies in the n & 3 tail: read as 0, and the counter moves by one (include/mmhip.h: once per thread that met one)"""
    lib = gu._lib.lib()
    cnt = torch.zeros(1, dtype=torch.int32, device=gu.dev())
    n = 4099
    p0, g0, m0, v0 = AR.make_state(n)
    g0[n - 1] = float("nan")
    bufs = _on_device((p0, g0, m0, v0))
    p, g, m, v = (b[1] for b in bufs)
    h = AR.hyper(1e-3, 0.01, 1, 1.0)
    g_read = g0.clone()
    g_read[n - 1] = 0.0
    ref, bound = AR.reference(p0, g_read, m0, v0, h)
    assert lib.mmhip_set_nonfinite_counter(gu.ptr(cnt)) == 0
    try:
        gu.call("mmhip_adamw", gu.ptr(p), gu.ptr(g), gu.ptr(m), gu.ptr(v), n, 1e-3, AR.BETA1, AR.BETA2, AR.EPS, 0.01, 1, 1.0, 1, gu.stream())
        torch.cuda.synchronize()
    finally:
        assert lib.mmhip_set_nonfinite_counter(None) == 0          # the process-wide registration must not outlive `cnt`
    assert int(cnt.item()) == 1
    _guards(bufs, "adamw tail")
    for name, got, r, b in zip("pmv", (p, m, v), ref, bound):
        gu.assert_close_elementwise(got, r, b, f"adamw tail-only non-finite: {name}")
