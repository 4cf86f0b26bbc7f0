"""-m gpu: global-norm gradient clipping (max_grad_norm) through the trainers -- late fusion with ITC + ITM, and one case each through the text-only
and the image-only trainer.  Tiny architectures, those of the tests whose helpers are used: late fusion as tests/test_gpu_model.py's _fresh_trainer (2 text + 1 image
layers, vocab 3000, B = 4, T = 32), text-only and image-only as the _case of tests/test_gpu_txt.py / test_gpu_img.py.  MMHIP_DETERMINISTIC=1 throughout: the native and the
staged step then produce the same gradient bits (tests/test_gpu_model.py), so a gradient taken from a staged backward of an identically seeded
trainer is the gradient the clipped native step saw.

One AdamW step from zero moments is almost invariant to the gradient's scale (m / sqrt(v) cancels it): the first step is judged on its MOMENTS
(m scales with coef, v with coef^2), parameters only after three steps."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adamw_ref as AR
import gpu_util as gu
import gradclip_ref as GR
from smtc_amd import _lib
from test_gpu_model import _fresh_trainer, _run_steps

DET = {"MMHIP_DETERMINISTIC": "1"}
LR, WD = 1e-3, 0.01          # what _run_steps passes


def _snapshot(tr):
    torch.cuda.synchronize()
    return tr.model._flat_train.clone(), tr._opt[0].clone(), tr._opt[1].clone(), tr.model._word_row_state.clone()


def _gradient_inputs(model, ranges, max_norm, gs=1.0):
    """tests/gradclip_ref.py inputs from what a backward left in `model`: the dense parts of `ranges` as segments, the word table and its flags"""
    g = model._flat_grad.cpu().numpy()
    word = model._word_info
    w0 = word["offset"] if word is not None else len(g)
    segs = [g[b: min(e, w0)] for b, e in ranges if min(e, w0) > b]
    table = state = None
    if word is not None and any(e > w0 for _, e in ranges):
        V, H = word["shape"]
        table, state = g[w0: w0 + V * H].reshape(V, H), model._word_row_state[:V].cpu().numpy()
    return GR.SimpleNamespace(segs=segs, table=table, state=state, gs=np.float32(gs), max_norm=np.float32(max_norm))


def _staged_gradient(tr, run):
    """one staged step of `tr` with the optimizer taken out: the gradient and the row flags stay in the model"""
    tr._adamw_ranges = lambda *a, **k: None
    run(tr)
    torch.cuda.synchronize()


def _check_first_step(tr, p0, inp, ranges, what):
    """after ONE clipped step from zero moments: reported norm and coef within the derived bounds of fp64 on the host; every element of p, m, v over
    the stepped ranges and flagged rows within tests/adamw_ref.py's bounds of the update on coef * g; everything else untouched"""
    ref = GR.reference(inp)
    st = tr.grad_clip_stats()
    print("margins", what, "k", ref.k, "norm", abs(st["norm"] - ref.total) / ref.b_total, "coef", abs(st["coef"] - ref.coef) / ref.b_coef, st)
    assert abs(st["norm"] - ref.total) <= ref.b_total, (what, st, ref.total, ref.b_total)
    assert abs(st["coef"] - ref.coef) <= ref.b_coef and 0.45 < st["coef"] < 0.55, (what, st, ref.coef, ref.b_coef)
    assert (st["clipped_steps"], st["steps"]) == (1, 1)
    m, dev = tr.model, tr.model._flat_train.device
    g = torch.from_numpy(np.concatenate([x.ravel() for x in inp.segs] + ([inp.table.ravel()] if inp.table is not None else []))).to(dev)
    word = m._word_info
    w0 = word["offset"] if word is not None else m._flat_train.numel()
    ar = lambda b, e: torch.arange(b, e, device=dev)
    idx = torch.cat([ar(b, min(e, w0)) for b, e in ranges if min(e, w0) > b] + ([ar(w0, w0 + word["numel"])] if inp.table is not None else []))
    stepped = torch.ones(len(idx), dtype=torch.bool, device=dev)
    if inp.table is not None:
        flagged = torch.from_numpy((inp.state & 1) != 0).to(dev)
        stepped[len(idx) - word["numel"]:] = flagged[:, None].expand(*word["shape"]).reshape(-1)
    p1, m1, v1 = m._flat_train, tr._opt[0], tr._opt[1]
    h = AR.hyper(LR, WD, 1, st["coef"])          # grad_scale is 1: the kernel multiplies by exactly the reported coefficient
    sel, gs = idx[stepped], g[stepped]
    zeros = torch.zeros(len(sel), device=dev)
    (rp, rm, rv), (bp, bm, bv) = AR.reference(p0[sel], gs, zeros, zeros, h)          # fp64, on the device: every stepped element, some twenty million

    def worst(got, r, b):
        err = (got.double() - r).abs()
        err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
        return torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf")))).max().item()
    margins = {n: worst(got[sel], r, b) for n, got, r, b in (("p", p1, rp, bp), ("m", m1, rm, bm), ("v", v1, rv, bv))}
    assert all(x <= 1.0 for x in margins.values()), (what, margins)
    # the closed forms the bounds stand for, and the proof that the check sees a missing clip: the unclipped moments lie outside
    c = st["coef"]
    assert torch.allclose(rm, (1 - h.b1) * c * gs.double(), rtol=1e-12, atol=0) and torch.allclose(rv, (1 - h.b2) * (c * gs.double()) ** 2, rtol=1e-12, atol=0)
    um, uv = (1 - h.b1) * gs.double(), (1 - h.b2) * gs.double() ** 2
    assert gu.violates_elementwise(um, rm, bm) > len(sel) // 2 and gu.violates_elementwise(uv, rv, bv) > len(sel) // 2
    # untouched: the inactive groups; unflagged word rows only take the decay
    rest = torch.ones(m._flat_train.numel(), dtype=torch.bool, device=dev)
    rest[sel] = False
    assert not bool(m1[rest].any()) and not bool(v1[rest].any()), f"{what}: moments outside the stepped ranges"
    inactive = rest.clone()
    if inp.table is not None:
        inactive[w0: w0 + word["numel"]] = False
        rows_off = idx[~stepped]
        decay = torch.tensor(1.0) - torch.tensor(LR) * torch.tensor(WD)
        assert torch.equal(p1[rows_off], p0[rows_off] * decay.to(dev)), f"{what}: unflagged rows take the decay alone"
    assert torch.equal(p1[inactive], p0[inactive]), f"{what}: parameters of inactive groups"
    print("margins", what, {k: round(x, 4) for k, x in margins.items()})


def test_reported_norm_and_moments_late_fusion():
    env = dict(DET)
    probe = _fresh_trainer()
    _staged_gradient(probe, lambda tr: _run_steps(tr, 1, dict(env, MMHIP_NATIVE_STEP="0")))
    mm = probe.model
    ranges = mm.active_ranges(True, True)
    assert len(ranges) <= GR.MAX_SEGMENTS
    unclipped = GR.reference(_gradient_inputs(mm, ranges, 1.0))
    inp = _gradient_inputs(mm, ranges, 0.5 * unclipped.total)
    # the norm is the sum over the NAMED active tensors: the <= 3 padding floats behind a tensor are zero
    g = mm._flat_grad.cpu().double()
    groups = mm.active_groups(True, True)
    named = sum(float((g[i["offset"]: i["offset"] + i["numel"]] ** 2).sum()) for i in mm._train_params if i["group"] in groups)
    for i in mm._train_params:
        pad = g[i["offset"] + i["numel"]: i["offset"] + ((i["numel"] + 3) & ~3)]
        assert not bool(pad.any()), i["name"]
    assert abs(named - unclipped.sum) <= 1e-12 * named and named > 0
    assert any(i["group"] not in groups for i in mm._train_params), "the layout has an inactive group to leave untouched"

    tr = _fresh_trainer()
    tr.set_max_grad_norm(float(inp.max_norm))
    p0 = tr.model._flat_train.clone()
    _run_steps(tr, 1, env)                                           # the native fused step
    _check_first_step(tr, p0, inp, ranges, "late fusion")


def _three_steps(env, max_grad_norm=None, disarm=False):
    tr = _fresh_trainer()
    if max_grad_norm is not None:
        tr.set_max_grad_norm(max_grad_norm)
    if disarm:
        tr.set_max_grad_norm(None)
    losses = _run_steps(tr, 3, dict(env, **DET))
    return tr, _snapshot(tr) + (losses,)


def test_a_threshold_that_never_clips_changes_no_bit():
    """max_grad_norm = 1e9: coef is exactly 1.0f, and three steps end on the parameters, moments, row flags and losses of an unarmed trainer whose
    AdamW launches all follow the backward (MMHIP_EARLY_ADAMW=0); disarming a trainer gives the same again"""
    _, plain = _three_steps({"MMHIP_EARLY_ADAMW": "0"})
    tr, armed = _three_steps({}, 1e9)
    for x, y in zip(plain, armed):
        assert torch.equal(x, y)
    st = tr.grad_clip_stats()
    assert st["coef"] == 1.0 and st["clipped_steps"] == 0 and st["steps"] == 3 and 0 < st["norm"] < 1e9
    tr2, disarmed = _three_steps({"MMHIP_EARLY_ADAMW": "0"}, 0.01, disarm=True)
    for x, y in zip(plain, disarmed):
        assert torch.equal(x, y)
    assert tr2.grad_clip_stats() is None and tr2.model._grad_clip is None


def test_clipped_native_and_staged_steps_agree_bitwise():
    a, native = _three_steps({}, 0.01)
    b, staged = _three_steps({"MMHIP_NATIVE_STEP": "0"}, 0.01)
    for x, y in zip(native, staged):
        assert torch.equal(x, y), (x.float() - y.float()).abs().max()
    for tr in (a, b):
        st = tr.grad_clip_stats()
        assert st["clipped_steps"] == 3 and st["steps"] == 3 and 0 < st["coef"] < 1 and st["norm"] > 0.01
    assert a.grad_clip_stats() == b.grad_clip_stats()
    _, plain = _three_steps({"MMHIP_EARLY_ADAMW": "0"})
    assert not torch.equal(native[0], plain[0]), "three clipped steps moved the parameters as three unclipped ones"


def test_a_void_f16_step_is_skipped_and_not_counted():
    """the overflow of tests/test_gpu_model.py test_step_guard_skips_a_void_step_as_a_whole, with clipping armed"""
    import types
    from smtc_amd.mm_late import MMLate_Model
    from smtc_amd.synthetic import synthetic_batch
    dev = torch.device("cuda:0")
    cfgd = types.SimpleNamespace(batch_size=4, num_labels=3, use_clip_loss=False, beta_itc=0.1, use_tim_loss=False, beta_itm=0.1, max_length=32, dropout=0.0)
    tr = MMLate_Model(cfgd, "bernice", "vit", "attention", arch=dict(layers_txt=2, layers_img=1, vocab=300, max_pos=130), seed=3, dtype="f16", max_grad_norm=0.01)
    mm = tr.model
    ids, mask, px, oh = synthetic_batch(mm.arch["vocab"], 3, 4, 32, 7, mm.arch["txt_kind"], mm.arch["pad_id"], True, mm.arch["image"], dev)
    tr.train_step(ids, mask, px, oh, None, 1e-3, 0.01, 1)
    before, st1 = _snapshot(tr), tr.grad_clip_stats()
    assert (st1["clipped_steps"], st1["steps"]) == (1, 1)
    mm._loss_scale = 2.0 ** 40
    _lib.check(_lib.lib().mmhip_set_loss_scale(mm._handle, mm._loss_scale))
    tr.train_step(ids, mask, px, oh, None, 1e-3, 0.01, 2)
    after, st2 = _snapshot(tr), tr.grad_clip_stats()
    assert int(mm._nonfinite[0].item()) > 0 and int(mm._nonfinite[1].item()) == 1
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    assert (st2["clipped_steps"], st2["steps"]) == (1, 1) and mm._flat_grad.abs().max().item() == 0.0


def test_refusals():
    lib = _lib.lib()
    tr = _fresh_trainer()
    mm = tr.model
    state = torch.zeros(int(lib.mmhip_grad_clip_state_bytes()), dtype=torch.uint8, device="cuda:0")
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert lib.mmhip_set_grad_clip(mm._handle, bad, _lib.ptr(state)) == -1
        with pytest.raises(ValueError):
            tr.set_max_grad_norm(bad)
    assert lib.mmhip_set_grad_clip(mm._handle, 1.0, C.c_void_p(state.data_ptr() + 4)) == -1 and lib.mmhip_set_grad_clip(None, 1.0, _lib.ptr(state)) == -1
    assert lib.mmhip_txt_set_grad_clip(mm._handle, 1.0, _lib.ptr(state)) == -1 and lib.mmhip_img_set_grad_clip(mm._handle, 1.0, _lib.ptr(state)) == -1      # a late-fusion handle
    with pytest.raises(ValueError):
        tr.set_max_grad_norm(0.0)
    assert mm._grad_clip is None and tr.grad_clip_stats() is None
    # the data-parallel step on an armed handle: MMHIP_E_STATE before anything is enqueued
    tr.set_max_grad_norm(0.5)
    from oracle import mm_oracle as O
    ids, mask, pixels, onehot = O.synthetic_batch(O.OracleConfig(layers_txt=2, layers_img=1, vocab=3000, max_pos=130, num_labels=3), 4, 32, 101, True)
    ids, mask, pixels, onehot = ids.cuda(), mask.cuda(), pixels.cuda().float().contiguous(), onehot.cuda().to(torch.int64).contiguous()
    tim = tr.prepare_itm_inputs(ids, mask)
    em, ev = tr._moments()
    loss = torch.full((4,), 7.0, device="cuda:0")
    ncorr = torch.full((1,), -7, dtype=torch.int32, device="cuda:0")
    calls = []
    cb = _lib.EXCHANGE_CB(lambda user, st: calls.append(st) or 0)
    p0 = _snapshot(tr)
    args = (mm._handle, _lib.ptr(ids), _lib.ptr(mask), _lib.ptr(pixels), _lib.ptr(tim[0]), _lib.ptr(tim[1]), _lib.ptr(tim[2]), _lib.ptr(onehot), None, 4, 32, 5, 1, 1,
            0.8, 0.1, 0.1, _lib.ptr(em), _lib.ptr(ev), LR, 0.9, 0.999, 1e-8, WD, 1, 1.0, _lib.ptr(loss), _lib.ptr(ncorr), _lib.stream_ptr())
    assert lib.mmhip_train_step_dp(*args, cb, None) == -2
    assert calls == [] and loss.tolist() == [7.0] * 4 and ncorr.item() == -7
    for x, y in zip(p0, _snapshot(tr)):
        assert torch.equal(x, y)
    assert tr.grad_clip_stats()["steps"] == 0
    # an armed step whose word table has no row flags: refused before its forward, nothing enqueued
    assert lib.mmhip_set_row_state(mm._handle, None) == 0
    assert lib.mmhip_train_step(*args) == -2 and loss.tolist() == [7.0] * 4 and ncorr.item() == -7
    assert lib.mmhip_set_row_state(mm._handle, _lib.ptr(mm._word_row_state)) == 0
    for x, y in zip(p0, _snapshot(tr)):
        assert torch.equal(x, y)
    # a forced exchange in one process is refused by the trainer as the constructor refuses a world size above 1
    from smtc_amd import dist as mmdist
    forced = mmdist.force_exchange
    mmdist.force_exchange = lambda: True
    try:
        with pytest.raises(NotImplementedError):
            tr.train_step(ids, mask, pixels, onehot, None, LR, WD, 1, tim=tim)
    finally:
        mmdist.force_exchange = forced
    tr.set_max_grad_norm(None)                                       # disarmed: the same call is taken
    assert lib.mmhip_train_step_dp(*args, cb, None) == 0 and calls
    torch.cuda.synchronize()
    assert loss[0].item() != 7.0


# ---------------------------------------------------------------------------------------------------------------- the one-tower trainers
def _one_tower(kind, max_grad_norm):
    if kind == "txt":
        from smtc_amd.text_only import TextModel
        from test_gpu_txt import KINDS, _case
        c = _case("xlmr")
        name, a = KINDS["xlmr"]

        class Cfg:
            batch_size, num_labels, max_length, dropout, use_loss_correction = 8, 3, 64, 0.1, False
        tm = TextModel(Cfg, name, arch=dict(a, layers=c["cfg"].layers_txt, vocab=c["cfg"].vocab), dtype="bf16", device="cuda:0", seed=3, max_grad_norm=max_grad_norm)
        tm.model.load_state_dict(c["P"], strict=False)
        return tm, lambda f, st: f(c["ids"], c["mask"], c["tt"], c["onehot"], c["w"], LR, WD, st, seed=1000 + st)
    from smtc_amd.image_only import ImageModel
    from test_gpu_img import _case
    c = _case(192, 2)
    tm = ImageModel(c["B"], 3, "vit", arch=dict(layers=c["cfg"].layers_img, image=c["image"]), dtype="bf16", device="cuda:0", seed=3, max_grad_norm=max_grad_norm)
    tm.model.load_state_dict(c["P"])
    return tm, lambda f, st: f(c["px"], c["onehot"], c["w"], LR, WD, st)


@pytest.mark.parametrize("kind", ["txt", "img"])
def test_one_tower_trainers(kind, monkeypatch):
    """run_txt's and run_img's trainers: the first step's reported norm and moments against the host, then three clipped steps native == staged"""
    monkeypatch.setenv("MMHIP_DETERMINISTIC", "1")
    probe, step = _one_tower(kind, None)
    _staged_gradient(probe, lambda tr: step(tr.staged_step, 1))
    ranges = probe.model.active_ranges()
    unclipped = GR.reference(_gradient_inputs(probe.model, ranges, 1.0))
    inp = _gradient_inputs(probe.model, ranges, 0.5 * unclipped.total)
    tm, step = _one_tower(kind, float(inp.max_norm))
    p0 = tm.model._flat_train.clone()
    step(tm.train_step, 1)
    torch.cuda.synchronize()
    _check_first_step(tm, p0, inp, ranges, kind)
    # three steps at a hundredth of the first norm, fused == staged bit for bit.  The count is pinned step by step against the reported norms (whose
    # accuracy the first-step check above established): at lr = 1e-3 these tiny models can fit their one batch within a step, after which the
    # gradient collapses by orders of magnitude and a later step may pass unclipped -- the text case clips all three
    res, max_norm = [], float(np.float32(0.01 * unclipped.total))
    for fused in (True, False):
        tm, step = _one_tower(kind, max_norm)
        norms = []
        for st in (1, 2, 3):
            step(tm.train_step if fused else tm.staged_step, st)
            norms.append(tm.grad_clip_stats()["norm"])
        want = sum(np.float32(max_norm) / (np.float32(x) + np.float32(1e-6)) < 1 for x in norms)
        stats = tm.grad_clip_stats()
        print("norms", kind, "fused" if fused else "staged", norms, "max_norm", max_norm, stats)
        assert (stats["clipped_steps"], stats["steps"]) == (want, 3) and norms[0] > max_norm and want >= 1, (norms, max_norm, stats)
        if kind == "txt":
            assert want == 3
        res.append((tm.model._flat_train.clone(), tm._opt[0].clone(), tm._opt[1].clone(), stats, norms))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2]) and res[0][3:] == res[1][3:]
