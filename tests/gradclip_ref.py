"""fp64 reference and derived bounds of global-norm gradient clipping (include/mmhip.h mmhip_op_grad_clip; csrc/gradnorm.hip), an fp32 emulation in
the kernels' order of summation and six wrong variants (numpy, no GPU: tests/test_gradclip_bounds_cpu.py checks the bounds,
tests/test_gpu_ops_gradclip.py and tests/test_gpu_gradclip.py the kernels and the trainers).

    S = sum g^2 over the dense segments and the rows whose state byte has bit0 (an element whose g * grad_scale is not finite adds 0)
    total = grad_scale * sqrt(S),    coef = min(1, max_norm / (total + 1e-6))                      (torch.nn.utils.clip_grad_norm_)

The kernels' summation tree (csrc/gradnorm.hip), which the bounds and the emulation follow:
    dense   BLOCKS workgroups of 256, NT threads in all.  Four-vector j * NT + t of a segment goes to accumulator j % 4 of thread t, element by element
            with a fused multiply-add; a segment's n & 3 tail elements go to accumulator 0 of threads 0 .. 2; the segments follow one another.
    rows    NW waves; 64-row chunk c belongs to wave c % NW, its flagged rows are taken in ascending order; four-vector 64 j + l of a row goes to
            accumulator j % 4 of lane l.
    both    a thread adds (a0 + a1) + (a2 + a3), six xor-shuffle steps add the 64 lanes, thread 0 adds the four waves (w0 + w1) + (w2 + w3): one
            fp32 partial per workgroup.  The finalize launch adds all partials in fp64 and forms total and coef in fp32.

Bounds (U = U_32; SLACK = 2 as in the other *_ref.py; nothing fitted).  All terms are non-negative, so k fp32 additions on the longest path of the
tree give |S' - S| <= gamma_k S with gamma_k = k U / (1 - k U),
    k = (the most fused multiply-adds any one accumulator performs) + REDUCE_DEPTH (2 + 6 + 2 additions behind it) + 1 (the square, were it rounded),
    total: gamma_k / 2 (the root halves a relative error) + 2 U (the fp64 tail rounded to fp32, once more for the fp64 sum and root);
    coef:  that + 3 U (the constant 1e-6f, the fp32 add, the fp32 division); min(1, .) widens nothing.  Where the quotient stays >= 1 under that
           relative error the coefficient must be exactly 1.0f (bound 0).
"""
import math
from types import SimpleNamespace

import numpy as np

from op_bounds import SLACK, U_32

BLOCKS, ROW_BLOCKS, THREADS, UNROLL, MAX_SEGMENTS = 512, 512, 256, 4, 16      # csrc/mmhip_kernels.h GRADNORM_*
NT = BLOCKS * THREADS                       # threads of the dense grid
PASS = NT * UNROLL * 4                      # elements one full trip of the dense main loop covers
NW = ROW_BLOCKS * THREADS // 64             # waves of the row grid
REDUCE_DEPTH = 2 + 6 + 2
EPS = 1e-6
FLT_MAX = float(np.finfo(np.float32).max)
F32 = np.float32
VARIANTS = ("no_grad_scale", "no_eps", "no_clamp", "not_rooted", "unflagged_rows", "tail_dropped")
MODES = ("half", "eps", "under")            # max_norm = half the norm | norm ~ 1e-5 and max_norm equal to it | above the norm; "zeros" is a case of its own

ROW_FLAGS_7 = [1, 0, 3, 2, 1, 0, 1]         # bit0 decides; 2 / 3 carry the "has moments" bit
SEG16 = [1, 2, 3, 4, 5, 7, 1020, 1024, 1027, 64, 300, 1, 8, 12, 2049, 513]
# name -> (dense segment sizes, (rows, width) or None, grad_scale, [(segment, index, value)] non-finite elements)
CASES = {f"n{n}": ([n], None, 1.0 if n % 2 else 0.5, []) for n in (1, 2, 3, 4, 5, 7, 1020, 1024, 1027)}
CASES.update({
    "pass-4": ([PASS - 4], None, 1.0, []), "pass": ([PASS], None, 0.5, []), "pass+7": ([PASS + 7], None, 1.0, []),
    "3pass+1027": ([3 * PASS + 1024 + 3], None, 0.5, []),
    "seg3": ([1027, 1, 4100], None, 0.5, []), "seg16": (SEG16, None, 1.0, []),
    "rows7x8": ([], (7, 8), 0.5, []), "rows1000x768": ([], (1000, 768), 1.0, []), "dense+rows": ([1027, 5], (1000, 768), 0.5, []),
    "nonfinite-body": ([1027], None, 1.0, [(0, 100, float("nan")), (0, 515, float("inf"))]),
    "nonfinite-tail": ([1027], None, 0.5, [(0, 1026, float("nan"))]),
})
BIG = ("pass-4", "pass", "pass+7", "3pass+1027")


def applies(variant, case, mode):
    """whether a wrong variant computes something else than the kernel for this case (read off the case, not off any result)"""
    if mode == "zeros":
        return variant == "no_clamp"
    segs, rows, gs, _ = CASES[case]
    return {"no_grad_scale": gs != 1.0, "no_eps": mode == "eps", "no_clamp": mode == "under", "not_rooted": True,
            "unflagged_rows": rows is not None, "tail_dropped": any(n & 3 for n in segs)}[variant]


ZERO_CASE = ([1027], (7, 8), 1.0, [])


def _flags(rows):
    if rows == 7:
        return np.array(ROW_FLAGS_7, dtype=np.uint8)
    rng = np.random.default_rng(77)
    st = (rng.integers(0, 2, rows) * 2).astype(np.uint8)                 # "has moments" bits at random: they must not matter
    st[rng.choice(rows, 37, replace=False)] |= 1
    st[[0, 63, 64, rows - 1]] |= 1                                       # both ends of a 64-row chunk, the last row
    st[[1, 65]] &= 0xFE
    return st


_BUILT = {}


def build(case, mode):
    """the inputs of one case: .segs (fp32 arrays), .table [rows, width] / .state (or None), .gs, .max_norm (fp32 values).  Unflagged rows hold NaN
    and 3e38 alternately: the kernel must not read them.  Each segment's tail elements carry about a hundredth of its sum of squares each, so that a
    dropped tail shows at every size.  Built once per (case, mode) and shared: treat as read-only."""
    if (case, mode) in _BUILT:
        return _BUILT[(case, mode)]
    seg_ns, rows, gs, bad = ZERO_CASE if mode == "zeros" else CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)) * 7919 + len(case))
    draw = lambda shape: (rng.standard_normal(shape) * 10.0 ** (-3 * rng.random(shape))).astype(F32)
    segs = []
    for n in seg_ns:
        x = draw(n)
        x[0] = F32(0.37) if x[0] == 0 else x[0]
        if n > 8:
            x[3::7] = 0.0
        n4 = n & ~3
        if n4 and n & 3:
            x[n4:] = F32(0.1 * math.sqrt(float((x[:n4].astype(np.float64) ** 2).sum()))) * np.array([1, -1, 1], dtype=F32)[: n & 3]
        segs.append(x)
    table = state = None
    if rows is not None:
        table, state = draw(rows), _flags(rows[0])
    inp = SimpleNamespace(case=case, mode=mode, segs=segs, table=table, state=state, gs=F32(gs), max_norm=F32(1.0))
    if mode == "zeros":
        for x in segs:
            x[:] = 0.0
        table[:] = 0.0
    else:
        for s, i, val in bad:
            segs[s][i] = val
        total0 = reference(inp).total
        assert total0 > 0
        if mode == "eps":                       # an exact power of two brings the norm to about 1e-5
            scale = F32(2.0 ** round(math.log2(1e-5 / total0)))
            for x in segs:
                x *= scale
            if table is not None:
                table *= scale
            inp.max_norm = F32(reference(inp).total)
        else:
            inp.max_norm = F32(0.5 * total0) if mode == "half" else F32(2.0 * total0 + 1.0)
    if table is not None:
        off = np.flatnonzero((state & 1) == 0)
        table[off[0::2]] = np.nan
        table[off[1::2]] = 3e38
    _BUILT[(case, mode)] = inp
    return inp


def _read(x, gs):
    """an element as the kernels read it: 0 where g * grad_scale is not finite in fp32"""
    with np.errstate(over="ignore", invalid="ignore"):
        ok = np.abs(x.astype(F32) * F32(gs)) <= F32(FLT_MAX)
    return np.where(ok, x, F32(0.0)).astype(F32)


def serial_adds(inp):
    """the most fused multiply-adds one accumulator performs: accumulator 0 of thread 0 (dense) / of a lane of the busiest wave (rows)"""
    kd = sum(4 * -(-(len(x) // 4) // (UNROLL * NT)) + (1 if len(x) & 3 else 0) for x in inp.segs)
    kr = 0
    if inp.table is not None:
        per_wave = np.bincount((np.flatnonzero(inp.state & 1) // 64) % NW, minlength=1)
        kr = int(per_wave.max()) * 4 * -(-(inp.table.shape[1] // 4) // (UNROLL * 64))
    return max(kd, kr)


def reference(inp, variant=None):
    """fp64: .sum, .total, .coef, .clipped and (variant None) the bounds .b_total, .b_coef; variant: one of VARIANTS (no bounds)"""
    gs, mx = float(inp.gs), float(inp.max_norm)
    S = 0.0
    for x in inp.segs:
        if variant == "tail_dropped":
            x = x[: len(x) & ~3]
        S += float((_read(x, gs).astype(np.float64) ** 2).sum())
    if inp.table is not None:
        t = inp.table if variant == "unflagged_rows" else inp.table[(inp.state & 1) != 0]
        S += float((_read(t, gs).astype(np.float64) ** 2).sum())
    root = S if variant == "not_rooted" else math.sqrt(S)
    total = root if variant == "no_grad_scale" else gs * root
    den = total if variant == "no_eps" else total + EPS
    q = mx / den if den > 0 else float("inf")
    coef = q if variant == "no_clamp" else min(1.0, q)
    r = SimpleNamespace(sum=S, total=total, coef=coef, clipped=coef < 1.0)
    if variant is None:
        k = serial_adds(inp) + REDUCE_DEPTH + 1
        gamma = k * U_32 / (1 - k * U_32)
        rel_total = gamma / 2 + 2 * U_32
        rel_coef = rel_total + 3 * U_32
        r.k = k
        r.b_total = SLACK * rel_total * total
        r.b_coef = 0.0 if q * (1 - SLACK * rel_coef) >= 1.0 else SLACK * rel_coef * q
    return r


def outside(inp, got_total, got_coef, ref=None):
    """whether (total, coef) leaves the bounds of the reference"""
    ref = ref or reference(inp)
    ok = lambda got, want, b: math.isfinite(got) and abs(got - want) <= b
    return not (ok(got_total, ref.total, ref.b_total) and ok(got_coef, ref.coef, ref.b_coef))


# ---------------------------------------------------------------------------------------------------------------- fp32 emulation in the kernels' order
def _fma_sq(acc, t):
    """fl32(t * t + acc): the square of an fp32 value is exact in fp64, the sum is then rounded to fp64 and to fp32 (a double rounding that differs
    from the fused operation in rare last-bit ties: the emulation is held to the bounds, not to the kernel's bits)"""
    t = t.astype(np.float64)
    return (t * t + acc.astype(np.float64)).astype(F32)


def _block_sums(acc):
    """[UNROLL, threads] accumulators -> one fp32 partial per 256 threads, in the kernels' order"""
    s = (acc[0] + acc[1]) + (acc[2] + acc[3])
    w = s.reshape(-1, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    ws = w[:, 0].reshape(-1, THREADS // 64)
    return (ws[:, 0] + ws[:, 1]) + (ws[:, 2] + ws[:, 3])


def emulate_partials(inp):
    parts = []
    live = [x for x in inp.segs if len(x)]
    if live:
        acc = np.zeros((UNROLL, NT), dtype=F32)
        for x in live:
            n, n4 = len(x), len(x) // 4
            v = _read(x[: n4 * 4], inp.gs).reshape(n4, 4)
            for j in range(-(-n4 // NT)):
                blk = v[j * NT: (j + 1) * NT]
                for e in range(4):
                    acc[j % UNROLL, : len(blk)] = _fma_sq(acc[j % UNROLL, : len(blk)], blk[:, e])
            if n & 3:
                acc[0, : n & 3] = _fma_sq(acc[0, : n & 3], _read(x[n4 * 4:], inp.gs))
        parts.append(_block_sums(acc))
    if inp.table is not None:
        acc = np.zeros((UNROLL, NW, 64), dtype=F32)
        nch = inp.table.shape[1] // 4
        for r in np.flatnonzero(inp.state & 1):
            w = (r // 64) % NW
            v = _read(inp.table[r], inp.gs).reshape(nch, 4)
            for j in range(-(-nch // 64)):
                blk = v[j * 64: (j + 1) * 64]
                for e in range(4):
                    acc[j % UNROLL, w, : len(blk)] = _fma_sq(acc[j % UNROLL, w, : len(blk)], blk[:, e])
        parts.append(_block_sums(acc.reshape(UNROLL, NW * 64)))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=F32)


def emulate(inp):
    """(total, coef, clipped) as fp32 values computed in the kernels' order"""
    p = emulate_partials(inp).astype(np.float64)
    p = np.concatenate([p, np.zeros(-len(p) % THREADS)]).reshape(-1, THREADS)
    s = np.zeros(THREADS)
    for row in p:
        s = s + row
    o = THREADS // 2
    while o:
        s[:o] = s[:o] + s[o: 2 * o]
        o //= 2
    total = F32(float(inp.gs) * math.sqrt(s[0]))
    q = F32(inp.max_norm) / (total + F32(EPS))
    coef = q if q < F32(1.0) else F32(1.0)
    return float(total), float(coef), bool(coef < F32(1.0))
