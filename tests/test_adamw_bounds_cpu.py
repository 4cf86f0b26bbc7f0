"""No GPU: the bounds of tests/adamw_ref.py hold for an fp32 computation in the kernels' order on every case tests/test_gpu_ops_adamw.py runs, and
four wrong variants leave them wherever they compute something else: the decay applied after the moment step, the bias corrections of step - 1, eps
inside the square root, grad_scale missing from the second moment."""
import itertools

import pytest
import torch

import adamw_ref as AR
from gpu_util import assert_close_elementwise, violates_elementwise

COMBOS = list(itertools.product(AR.STEPS, AR.GRAD_SCALES))


@pytest.mark.parametrize("lr,wd", AR.LR_WD)
@pytest.mark.parametrize("n", AR.NS + [7 * w for w in AR.ROW_WIDTHS])
def test_fp32_computation_stays_inside(n, lr, wd):
    p, g, m, v = AR.make_state(n)
    for step, gs in COMBOS:
        h = AR.hyper(lr, wd, step, gs)
        ref, bound = AR.reference(p, g, m, v, h)
        emu = AR.emulate(p, g, m, v, h)
        for name, e, r, b in zip("pmv", emu, ref, bound):
            assert assert_close_elementwise(e, r, b, f"emulated {name} n={n} step={step} gs={gs}") <= 1


@pytest.mark.parametrize("lr,wd", AR.LR_WD)
@pytest.mark.parametrize("n", AR.NS)
def test_wrong_variants_leave_the_bounds(n, lr, wd):
    p, g, m, v = AR.make_state(n)
    for step, gs in COMBOS:
        h = AR.hyper(lr, wd, step, gs)
        ref, bound = AR.reference(p, g, m, v, h)
        for variant in AR.VARIANTS:
            if not AR.applies(variant, h):
                continue
            wrong = AR.reference(p, g, m, v, h, variant=variant)
            # (a NaN -- step - 1 = 0 divides by a zero bias correction -- fails assert_close_elementwise as well; violates_elementwise skips it)
            out = sum(violates_elementwise(w, r, b) + int((~torch.isfinite(w)).sum()) for w, r, b in zip(wrong, ref, bound))
            what = f"{variant} n={n} step={step} gs={gs} lr={lr} wd={wd}"
            assert out > 0, what


def test_rows_reference_follows_the_state_bytes():
    """the row form's expectations: untouched gradient rows, cleared ones, the state transitions, decay-only rows exact"""
    h = AR.hyper(1e-3, 0.01, 2, 0.5)
    p, g, m, v, st = AR.rows_state(4)
    for zg in (0, 1):
        ref, bound, idle, exact_p, st_after, g_after = AR.rows_reference(p, g, m, v, st, h, zg)
        assert idle.tolist() == [s == 0 for s in AR.ROW_STATES]
        assert st_after.tolist() == [0 if s == 0 else (2 | (0 if zg else s & 1)) for s in AR.ROW_STATES]
        for r, s in enumerate(AR.ROW_STATES):
            assert torch.equal(g_after[r], torch.zeros(4) if (zg and s & 1) else g[r])
        assert assert_close_elementwise(exact_p[idle], ref[0][idle], bound[0][idle], "decay-only rows") <= 1
    assert set(AR.ROW_STATES) == {0, 1, 2, 3} and len(AR.ROW_STATES) % 4


def test_big_case_stays_inside_and_wrong_variants_leave():
    """the one large GPU case, with the hyper-parameters it runs at"""
    h = AR.hyper(1e-3, 0.01, 2, 0.5)
    state = AR.make_state_on(AR.BIG_N, "cpu")
    ref, bound = AR.reference(*state, h)
    for name, e, r, b in zip("pmv", AR.emulate(*state, h), ref, bound):
        assert assert_close_elementwise(e, r, b, f"emulated {name} n={AR.BIG_N}") <= 1
    for variant in AR.VARIANTS:
        wrong = AR.reference(*state, h, variant=variant)
        assert sum(violates_elementwise(w, r, b) for w, r, b in zip(wrong, ref, bound)) > 0, variant


def test_big_case_is_the_smallest_that_loops_twice():
    blocks = lambda n: min((n // 4 + 255) // 256, 16384)
    assert (AR.BIG_N // 4) > blocks(AR.BIG_N) * 256 and AR.BIG_N & 3 == 3
    n = AR.BIG_N - 1024 - 3 + 3          # one 256-vector workgroup less: a single pass
    assert (n // 4) <= blocks(n) * 256
