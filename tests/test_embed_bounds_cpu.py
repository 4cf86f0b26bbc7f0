"""No GPU: the bounds of tests/embed_ref.py are neither too narrow nor uselessly wide.
  * an fp32 emulation of the embedding kernels' arithmetic order (fp32 sums, xhat and x rounded as stored, the scatter in a random order) stays INSIDE
    every bound on every case tests/test_gpu_ops_embed.py runs, for every dtype: the inputs were chosen so that a correct kernel passes;
  * each deliberately wrong variant -- a word row that loses one slot, a gradient in the padding_idx row, XLM-R position ids that count a pad, the keep
    mask one element late, type-0 tokens in row 1, alpha twice on the position rows, dbeta from the undropped gradient, type row 0 for id 1 -- lands
    OUTSIDE at least one element's bound, for every dtype's bound.
The second point is what makes a passing -m gpu run mean something."""
import pytest
import torch

import embed_ref as ER
from gpu_util import assert_close_elementwise, violates_elementwise
from op_bounds import pair_hi_is_nearest

DTYPES = ["bf16", "f16", "x3"]
BWD_OUT = ("dword", "dpos", "dtype", "dgamma", "dbeta", "det_rows")


@pytest.mark.parametrize("k", range(len(ER.VARIANTS)))
@pytest.mark.parametrize("shape", ER.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_emulated_kernels_stay_inside_every_bound(shape, k):
    c = ER.case_of(shape, k)
    fr = ER.fwd_reference(c, c.p, c.seed)
    keep, scale = ER.keep_of(c, c.p, c.seed)
    for dt in DTYPES:
        fb = ER.fwd_bounds(c, fr, dt)
        pid, mb, xhat, rstd, x, (hi, lo) = ER.emulate_fwd(c, c.p, c.seed, dt)
        assert torch.equal(pid, fr.pos_ids) and torch.equal(mb.double(), fr.maskbias)
        for name, got in (("xhat", xhat), ("rstd", rstd), ("x", x)):
            assert assert_close_elementwise(got, getattr(fr, name), fb[name], f"emulated {name} {dt}") <= 1
        if dt == "x3":
            assert assert_close_elementwise(hi.double() + lo.double(), fr.x, fb["x_pair"], "emulated x_pair") <= 1 and pair_hi_is_nearest(hi, lo).all()
        assert (fb["x"][fr.ks == 0] == 0).all()                      # dropped elements: exactly 0 is required
        bi = ER.bwd_inputs(c, fr, dt)
        ref, b = ER.bwd_reference(c, bi, keep, scale, c.alpha)
        emu = ER.emulate_bwd(c, bi, keep, scale, c.alpha, perm_seed=k)
        for name in BWD_OUT:
            assert assert_close_elementwise(emu[name], ref[name], b[name], f"emulated {name} {dt}") <= 1


@pytest.mark.parametrize("dt", DTYPES)
def test_emulated_deterministic_scatter_stays_inside(dt):
    c = ER.case_of((17, 65, 768), 2)
    fr = ER.fwd_reference(c, c.p, c.seed)
    keep, scale = ER.keep_of(c, c.p, c.seed)
    bi = ER.bwd_inputs(c, fr, dt)
    ref, b = ER.bwd_reference(c, bi, keep, scale, c.alpha)
    emu = ER.emulate_bwd(c, bi, keep, scale, c.alpha, deterministic=True)
    for name in BWD_OUT:
        assert assert_close_elementwise(emu[name], ref[name], b[name], f"deterministic {name} {dt}") <= 1


def test_rows_that_must_keep_their_prefill_have_bound_zero():
    """the padding_idx rows, the rows no slot names, row 0 of dtype in the one-row mode, row 1 without type ids: bound 0, reference == prefill"""
    for k, tt in ((1, "one"), (3, "none"), (7, "one"), (5, "two")):
        c = ER.case_of((5, 3, 132), k)
        assert c.tt == tt
        fr = ER.fwd_reference(c, c.p, c.seed)
        keep, scale = ER.keep_of(c, c.p, c.seed)
        ref, b = ER.bwd_reference(c, ER.bwd_inputs(c, fr, "bf16"), keep, scale, c.alpha)
        unnamed = torch.ones(c.vocab, dtype=torch.bool)
        unnamed[c.ids[c.ids != c.pad]] = False
        assert unnamed[c.pad] and unnamed.sum() > 1
        assert (b["dword"][unnamed] == 0).all() and torch.equal(ref["dword"][unnamed], c.pre["dword"].double()[unnamed])
        assert (b["dword"][~unnamed] > 0).all()
        if c.xlmr:
            assert (b["dpos"][c.pad] == 0).all() and torch.equal(ref["dpos"][c.pad], c.pre["dpos"].double()[c.pad])
        else:
            assert (b["dpos"][0] > 0).all()
        fixed = {"none": 1, "one": 0}.get(tt)
        if fixed is not None:
            assert (b["dtype"][fixed] == 0).all() and torch.equal(ref["dtype"][fixed], c.pre["dtype"].double()[fixed])
        assert (b["dtype"][1 if tt != "none" else 0] > 0).all()


def test_entry_points_reject_on_the_host():
    """no device pointer is dereferenced and nothing is launched for an argument outside the limits (no GPU here: a launch would fail differently)"""
    import ctypes as C
    from smtc_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.lib()
    one, odd = C.c_void_p(256), C.c_void_p(260)

    def fwd(**kw):
        a = dict(dtype=2, ids=one, mask=one, type_ids=None, word=one, pos=one, type=one, gamma=one, beta=one, eps=1e-5, posts=2, T=3, H=8, xlmr=1, pad_id=1, p=0.1,
                 seed=1, x=one, xhat=one, rstd=one, pos_ids=one, maskbias=one, x_pair=None, ld_pair=16, lo_pair=8)
        a.update(kw)
        return lib.mmhip_op_embed_fwd(*a.values(), None)

    def bwd(**kw):
        a = dict(dtype=2, dx=one, xhat=one, rstd=one, gamma=one, ids=one, pos_ids=one, type_ids=None, type_rows=0, posts=2, T=3, H=8, pad_id=1, pos_pad_id=1, p=0.1,
                 seed=1, alpha=0.0, dword=one, dpos=one, dtype_rows=one, dgamma=one, dbeta=one, partial=None, partial_bytes=0, row_state=None, det_rows=None,
                 max_pos=0, status=None)
        a.update(kw)
        return lib.mmhip_op_embed_bwd(*a.values(), None)

    for bad in (dict(ids=None), dict(mask=None), dict(word=None), dict(pos=None), dict(type=None), dict(gamma=None), dict(beta=None), dict(x=None), dict(pos_ids=None),
                dict(maskbias=None), dict(posts=0), dict(T=0), dict(H=0), dict(H=6), dict(H=1028), dict(p=-0.1), dict(p=1.0), dict(p=float("nan")), dict(dtype=3),
                dict(word=odd), dict(pos=odd), dict(type=odd), dict(gamma=odd), dict(beta=odd), dict(x=odd), dict(xhat=odd), dict(x_pair=odd), dict(dtype=0, x_pair=one),
                dict(x_pair=one, lo_pair=4), dict(x_pair=one, ld_pair=12), dict(x_pair=one, lo_pair=10, ld_pair=20)):
        assert fwd(**bad) == -1, bad
    for bad in (dict(dx=None), dict(xhat=None), dict(rstd=None), dict(gamma=None), dict(ids=None), dict(pos_ids=None), dict(dword=None), dict(dpos=None),
                dict(dtype_rows=None), dict(dgamma=None), dict(dbeta=None), dict(posts=0), dict(T=0), dict(H=0), dict(H=6), dict(H=1028), dict(p=-0.1), dict(p=1.0),
                dict(dtype=3), dict(type_rows=2), dict(det_rows=one, max_pos=0), dict(dx=odd), dict(xhat=odd), dict(gamma=odd), dict(det_rows=odd, max_pos=8),
                dict(row_state=C.c_void_p(257)), dict(status=C.c_void_p(258))):
        assert bwd(**bad) == -1, bad
    nblk = 3 * 1
    assert lib.mmhip_op_embed_bwd_ws_bytes(2, 3, 8, 0) == 3 * nblk * 8 * 4 and lib.mmhip_op_embed_bwd_ws_bytes(2, 3, 8, 2) == 4 * nblk * 8 * 4
    assert lib.mmhip_op_embed_bwd_ws_bytes(17, 65, 768, 1) == 3 * 65 * 2 * 768 * 4 and lib.mmhip_op_embed_bwd_ws_bytes(0, 3, 8, 0) == 0
    assert bwd(partial=one, partial_bytes=3 * nblk * 8 * 4 - 1) == -3
    assert bwd(partial=one, partial_bytes=3 * nblk * 8 * 4, type_rows=2, type_ids=one) == -3


def _mutant_case(tt):
    c = ER.make_case(5, 7, 132, ER.SMALL_VOCAB, "middle", 1, tt, seed=11)
    c.p, c.alpha, c.seed = 0.1, 0.37, ER.DROP_SEED
    return c


@pytest.mark.parametrize("dt", DTYPES)
def test_wrong_backward_variants_leave_the_bounds(dt):
    for tt in ("one", "two"):
        c = _mutant_case(tt)
        fr = ER.fwd_reference(c, c.p, c.seed)
        keep, scale = ER.keep_of(c, c.p, c.seed)
        bi = ER.bwd_inputs(c, fr, dt)
        ref, b = ER.bwd_reference(c, bi, keep, scale, c.alpha)
        assert (c.ids == c.pad).any() and (c.type_ids == 0).any()
        for mutant, seen_in in (("drop_word_slot", "dword"), ("pad_row", "dword"), ("keep_shift", "dword"), ("keep_shift", "dbeta"),
                                ("type0_into_row1", "dtype"), ("alpha_twice_pos", "dpos"), ("dbeta_raw", "dbeta")):
            wrong, _ = ER.bwd_reference(c, bi, keep, scale, c.alpha, mutant=mutant, with_bounds=False)
            assert violates_elementwise(wrong[seen_in], ref[seen_in], b[seen_in]) > 0, (tt, mutant, seen_in)
        wrong, _ = ER.bwd_reference(c, bi, keep, scale, c.alpha, mutant="pad_row", with_bounds=False)
        assert violates_elementwise(wrong["dword"][c.pad], ref["dword"][c.pad], b["dword"][c.pad]) > 0          # seen IN the padding_idx row


@pytest.mark.parametrize("dt", DTYPES)
def test_wrong_forward_variants_leave_the_bounds(dt):
    c = _mutant_case("two")
    fr = ER.fwd_reference(c, c.p, c.seed)
    fb = ER.fwd_bounds(c, fr, dt)
    live = c.ids != c.pad
    assert (~live[:, 1:-1]).any()                                  # a pad inside a post
    w = ER.fwd_reference(c, c.p, c.seed, mutant="pos_no_skip")
    assert not torch.equal(w.pos_ids, fr.pos_ids)                  # exact output: any difference is a failure
    w2 = ER.fwd_reference(c, c.p, c.seed, mutant="type_row0")
    for wrong in (w, w2):
        for name in ("x", "xhat"):
            assert violates_elementwise(getattr(wrong, name), getattr(fr, name), fb[name]) > 0, name
    assert violates_elementwise(w2.x, fr.x, fb["x_pair"]) > 0
