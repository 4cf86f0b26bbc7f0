"""Text-only path on the GPU: the fused CLS classifier head against fp64 with per-element bounds, the BERT / BERNICE drop-ins against the fp32
restatement of the reference modules (tests/txt_ref.py; dropout masks replayed), the fused step against the staged one, the command line.

Tolerances of the model tests are the ones tests/test_gpu_model.py holds the late-fusion model to at two layers (imported, not restated)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mm_oracle as O
from smtc_amd import _lib
import op_bounds as OB
import txt_ref as R
from test_gpu_model import TOL_OUT, TOL_GRAD, TOL_LOSS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
DT = {"bf16": _lib.BF16, "f16": _lib.F16, "f32": _lib.F32, "pair": 3}


# ------------------------------------------------------------------------------------------------ the head's two launches alone
def _store_rows(x64, B, stride, H, name):
    """CLS rows [B, H] (fp64) as the engine stores them, row b at element b * stride; -> (device tensor, the values as the kernel reads them)"""
    if name in ("bf16", "f16"):
        td = torch.bfloat16 if name == "bf16" else torch.float16
        buf = torch.full((B * stride,), 7.0, dtype=td)
        rows = x64.to(td)
        buf.view(B, stride)[:, :H] = rows
        return buf.to(DEV), rows.double()
    if name == "f32":
        buf = torch.full((B * stride,), 7.0)
        buf.view(B, stride)[:, :H] = x64.float()
        return buf.to(DEV), x64.float().double()
    hi, lo = OB.split_pair(x64)                       # pair row: [hi(H) | lo(H)] in the bytes of the fp32 row; stride counts 4-byte elements
    buf = torch.full((B * stride * 2,), 7.0, dtype=torch.bfloat16)
    v = buf.view(B, 2 * stride)
    v[:, :H], v[:, H:2 * H] = hi, lo
    return buf.to(DEV), hi.double() + lo.double()


@pytest.mark.parametrize("name", ["bf16", "f16", "f32", "pair"])
def test_cls_head_ops_per_element(name):
    """B in {1, 3, 64, 65} x C in {2, 3, 16}, H = 768, compact and T*H strides, dropout off and on: every element of logits, d logits, dW, db, dx
    within the bound of an fp32 sum of its length on sum |a||b| (op_bounds: K * U_32, SLACK 2); loss and count; dW bit-identical across two calls."""
    lib, H, T, seed = _lib.lib(), 768, 4, 0x1234567887654321
    s = _lib.stream_ptr()
    g = torch.Generator().manual_seed(5)
    for B in (1, 3, 64, 65):
        for Cn in (2, 3, 16):
            for stride in (H, T * H):
                for p in (0.0, 0.1):
                    x64 = torch.randn(B, H, generator=g, dtype=torch.float64)
                    W = (0.05 * torch.randn(Cn, H, generator=g)).float()
                    bias = (0.1 * torch.randn(Cn, generator=g)).float()
                    cw = (0.5 + torch.rand(Cn, generator=g)).float()
                    onehot = torch.eye(Cn, dtype=torch.int64)[torch.randint(0, Cn, (B,), generator=g)]
                    xd_dev, xr = _store_rows(x64, B, stride, H, name)
                    keep = torch.from_numpy(O.hash_keep_mask(B * H, 0, O.STREAM_HEAD, seed, p)).view(B, H) if p > 0 else torch.ones(B, H, dtype=torch.bool)
                    ks = float(torch.tensor(O.keep_scale(p) if p > 0 else 1.0, dtype=torch.float32))
                    xd = xr * keep.double() * ks
                    Wd, bd = W.double(), bias.double()
                    z = xd @ Wd.t() + bd
                    zb = OB.SLACK * (H + 2) * OB.U_32 * (xd.abs() @ Wd.abs().t() + bd.abs()) + 1e-30
                    lsm = torch.log_softmax(z, dim=1)
                    y, cwd = onehot.double(), cw.double()
                    loss = -(y * lsm * cwd).sum() / B
                    wy = (y * cwd).sum(dim=1, keepdim=True)
                    dl = (torch.softmax(z, dim=1) * wy - cwd * y) / B
                    Wg, bg, cwg, ohg = W.to(DEV), bias.to(DEV), cw.to(DEV), onehot.to(DEV)
                    logits = torch.empty(B, Cn, device=DEV)
                    dlg = torch.empty(B, Cn, device=DEV)
                    lossg = torch.empty(1, device=DEV)
                    ncg = torch.empty(1, dtype=torch.int32, device=DEV)
                    _lib.check(lib.mmhip_op_cls_head_fwd(DT[name], _lib.ptr(xd_dev), stride, _lib.ptr(Wg), _lib.ptr(bg), B, Cn, H, p, seed, _lib.ptr(logits),
                                                         _lib.ptr(ohg), _lib.ptr(cwg), _lib.ptr(lossg), _lib.ptr(ncg), _lib.ptr(dlg), s), "cls_head_fwd")
                    plain = torch.empty(B, Cn, device=DEV)
                    _lib.check(lib.mmhip_op_cls_head_fwd(DT[name], _lib.ptr(xd_dev), stride, _lib.ptr(Wg), _lib.ptr(bg), B, Cn, H, p, seed, _lib.ptr(plain),
                                                         None, None, None, None, None, s), "cls_head_fwd")
                    tag = (name, B, Cn, stride, p)
                    got = logits.cpu().double()
                    assert ((got - z).abs() <= zb).all(), (tag, ((got - z).abs() / zb).max())
                    assert torch.equal(plain, logits), tag          # the label-free launch (many blocks) computes the same logits
                    # softmax of logits that are each off by <= zb, through v_exp_f32 / v_log_f32 (SLACK), C terms: first order 2 max zb per element
                    dlb = (2 * zb.max(dim=1, keepdim=True).values + OB.SLACK * (Cn + 4) * OB.U_32) * (wy + cwd) / B
                    assert ((dlg.cpu().double() - dl).abs() <= dlb).all(), tag
                    lb = (2 * zb.max() + OB.SLACK * (Cn + 4 + math.log2(B + 1)) * OB.U_32 * (1 + z.abs().max())) * cwd.max() * (1 + B * OB.U_32)
                    assert abs(float(lossg) - float(loss)) <= float(lb) * max(1.0, float(loss.abs())), (tag, float(lossg), float(loss))
                    margin = z.sort(dim=1).values
                    sure = (margin[:, -1] - margin[:, -2]) > 2 * zb.max()
                    want_c = (z.argmax(dim=1) == onehot.argmax(dim=1))
                    assert abs(int(ncg) - int(want_c.sum())) <= int((~sure).sum()), tag
                    # ---- backward from the kernel's own d logits (fp32 values, exact in fp64)
                    dlr = dlg.cpu().double()
                    for odt, oname in ((_lib.F32, "f32"), (DT[name] if name in ("bf16", "f16") else _lib.F32, name)):
                        sc = 1024.0 if oname == "f16" else 1.0
                        td = {"bf16": torch.bfloat16, "f16": torch.float16}.get(oname, torch.float32)
                        u_out = {"bf16": OB.U_BF16, "f16": OB.U_F16}.get(oname, OB.U_32)
                        dW = torch.full((Cn, H), 3.0, device=DEV)
                        db = torch.full((Cn,), 3.0, device=DEV)
                        dx = torch.full((B * stride,), 5.0, dtype=td, device=DEV)
                        args = (DT[name], _lib.ptr(xd_dev), stride, _lib.ptr(Wg), _lib.ptr(dlg), B, Cn, H, p, seed)
                        _lib.check(lib.mmhip_op_cls_head_bwd(*args, _lib.ptr(dW), _lib.ptr(db), odt, _lib.ptr(dx), stride, sc, 0, s), "cls_head_bwd")
                        dW2 = torch.full((Cn, H), -1.0, device=DEV)
                        _lib.check(lib.mmhip_op_cls_head_bwd(*args, _lib.ptr(dW2), None, odt, None, 0, sc, 0, s), "cls_head_bwd")
                        assert torch.equal(dW, dW2), tag
                        rW, rb = dlr.t() @ xd, dlr.sum(dim=0)
                        bW = OB.SLACK * (B + 2) * OB.U_32 * (dlr.abs().t() @ xd.abs()) + 1e-30
                        assert ((dW.cpu().double() - rW).abs() <= bW).all(), (tag, oname)
                        assert ((db.cpu().double() - rb).abs() <= OB.SLACK * (B + 1) * OB.U_32 * dlr.abs().sum(dim=0) + 1e-30).all(), (tag, oname)
                        rx = (dlr @ Wd) * keep.double() * ks * sc
                        bx = (OB.SLACK * (Cn + 3) * OB.U_32 + u_out) * (dlr.abs() @ Wd.abs()) * ks * sc + 1e-30
                        gx = dx.view(B, stride).cpu().double()
                        assert ((gx[:, :H] - rx).abs() <= bx).all(), (tag, oname)
                        if stride > H:
                            assert (gx[:, H:] == 5.0).all(), (tag, oname)          # nothing outside the CLS rows is written
                        acc = torch.full((Cn, H), 0.25, device=DEV)                 # accumulate: added to what is there, still one writer
                        _lib.check(lib.mmhip_op_cls_head_bwd(*args, _lib.ptr(acc), None, odt, None, 0, sc, 1, s), "cls_head_bwd")
                        assert torch.equal(acc, dW + 0.25) or ((acc.cpu().double() - 0.25 - rW).abs() <= bW + 0.25 * OB.U_32 * 2).all(), tag


def test_cls_head_rejects_shapes():
    lib, s = _lib.lib(), _lib.stream_ptr()
    x = torch.zeros(4 * 768, device=DEV)
    W, b, out = torch.zeros(17 * 768, device=DEV), torch.zeros(17, device=DEV), torch.zeros(4 * 17, device=DEV)
    f = lambda B, Cn, H, stride: lib.mmhip_op_cls_head_fwd(_lib.F32, _lib.ptr(x), stride, _lib.ptr(W), _lib.ptr(b), B, Cn, H, 0.0, 0, _lib.ptr(out),
                                                           None, None, None, None, None, s)
    assert f(4, 17, 768, 768) == -1 and f(4, 3, 736, 736) == -1 and f(0, 3, 768, 768) == -1 and f(4, 3, 768, 704) == -1 and f(4, 3, 768, 768) == 0


# ------------------------------------------------------------------------------------------------ the modules
KINDS = {"xlmr": ("bernice", dict(txt_kind="xlmr", max_pos=130, type_vocab=1, pad_id=1, ln_eps_txt=1e-5)),
         "bert": ("bert", dict(txt_kind="bert", max_pos=128, type_vocab=2, pad_id=0, ln_eps_txt=1e-12))}
_REF = {}


def _case(kind, B=4, T=32, seed_x=7):
    """inputs (padded rows; BERT: non-zero token types on some tokens), weights and class weights -- computed once, shared, never changed"""
    key = (kind, B, T, seed_x)
    if key not in _REF:
        cfg = R.oracle_cfg(kind=kind)
        ids, mask, _, onehot = O.synthetic_batch(O.OracleConfig(**{**cfg.__dict__, "image": 16}), B, T, seed_x, True)
        tt = None
        if kind == "bert":
            tt = torch.zeros(B, T, dtype=torch.int64)
            tt[:, T // 3:] = 1
            tt[1] = 0
            tt = tt * mask
        _REF[key] = dict(cfg=cfg, ids=ids, mask=mask, tt=tt, onehot=onehot, w=torch.tensor([1.0, 2.0, 0.5]), P=R.make_params(cfg, 0))
    return _REF[key]


def _model(kind, dtype, c, B=8, T=64, dropout=None):
    from smtc_amd.text_only import BERT, BERNICE
    cfg = c["cfg"]
    name, a = KINDS[kind]
    arch = dict(a, layers=cfg.layers_txt, vocab=cfg.vocab, p_hidden=cfg.p_hidden, p_attn=cfg.p_attn)
    m = (BERNICE if kind == "xlmr" else BERT)("", cfg.num_labels, cfg.p_head if dropout is None else dropout, arch=arch, arch_name=name, dtype=dtype,
                                              max_posts=B, max_text_len=T, device=DEV)
    sd = m.state_dict()
    assert set(c["P"]) | {"bert_model.embeddings.position_ids"} == set(sd)
    assert all(tuple(sd[k].shape) == tuple(v.shape) for k, v in c["P"].items())
    missing, unexpected = m.load_state_dict(c["P"], strict=False)
    assert unexpected == [] and missing == ["bert_model.embeddings.position_ids"]
    return m


def _call(m, c, kind):
    return m(c["ids"], c["mask"]) if kind == "xlmr" else m(c["ids"], c["mask"], c["tt"])


def _ref_eval(c):
    if "eval" not in c:
        with torch.no_grad():
            c["eval"] = R.forward(c["P"], c["ids"], c["mask"], c["tt"], c["cfg"])
    return c["eval"]


@pytest.mark.parametrize("dtype", ["bf16x3", "bf16", "f16"])
@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_eval_logits(kind, dtype):
    c = _case(kind)
    m = _model(kind, dtype, c)
    m.eval()
    with torch.no_grad():
        out = _call(m, c, kind).cpu()
    ref = _ref_eval(c)
    err = (out - ref).abs().max().item() / ref.abs().max().item()
    print(f"eval logits {kind} {dtype}: {err:.3e}")
    assert err < TOL_OUT[dtype]["out_cls"]


@pytest.mark.parametrize("dtype", ["bf16x3", "bf16", "f16"])
@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_eval_logits_against_reference_golden(kind, dtype):
    """the logits the reference's own BERNICE / BERT computed (tests/golden/make_txt_golden.py): 1e-3 in bf16x3, the 16-bit bands otherwise"""
    import ast
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", f"txt_small_{kind}.npz"), allow_pickle=False)
    cfg = O.OracleConfig(**ast.literal_eval(str(z["cfg"])))
    t = lambda k: torch.from_numpy(z[k])
    c = dict(cfg=cfg, ids=t("ids"), mask=t("mask"), tt=t("token_type_ids") if kind == "bert" else None, P=R.make_params(cfg, 0))
    m = _model(kind, dtype, c)
    m.eval()
    with torch.no_grad():
        out = _call(m, c, kind).cpu()
    err = (out - t("logits")).abs().max().item() / t("logits").abs().max().item()
    print(f"eval logits vs reference golden {kind} {dtype}: {err:.3e}")
    assert err < TOL_OUT[dtype]["out_cls"]


def _watched(cfg, c):
    w = ["linear.weight", "linear.bias", "bert_model.embeddings.LayerNorm.weight", "bert_model.embeddings.LayerNorm.bias",
         "bert_model.embeddings.position_embeddings.weight", "bert_model.embeddings.word_embeddings.weight",
         "bert_model.embeddings.token_type_embeddings.weight"]
    for l in range(cfg.layers_txt):
        p = f"bert_model.encoder.layer.{l}."
        w += [p + n for n in ("attention.self.query.weight", "attention.self.query.bias", "attention.self.value.weight", "attention.output.dense.weight",
                              "attention.output.LayerNorm.weight", "intermediate.dense.weight", "intermediate.dense.bias", "output.dense.weight",
                              "output.LayerNorm.bias")]
    return w


@pytest.mark.parametrize("dtype", ["bf16x3", "bf16", "f16"])
@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_gradients_with_dropout(kind, dtype):
    """loss.backward() on the returned logits, dropout on (the restatement replays the masks from the step's seed): per-tensor relative L2"""
    c = _case(kind)
    cfg = c["cfg"]
    m = _model(kind, dtype, c)
    m.train()
    logits = _call(m, c, kind)
    loss = O.cls_loss(logits, c["onehot"].to(DEV), c["w"].to(DEV))
    loss.backward()
    r_logits, r_loss, G = R.loss_and_grads(c["P"], c["ids"], c["mask"], c["tt"], c["onehot"], c["w"], cfg, O.Dropout("hash", m._last["seed"]))
    e_loss = abs(loss.item() - r_loss.item()) / abs(r_loss.item())
    print(f"train loss {kind} {dtype}: {loss.item():.6f} vs {r_loss.item():.6f} ({e_loss:.2e})")
    assert e_loss < (TOL_LOSS[dtype] if dtype == "bf16x3" else TOL_OUT[dtype]["out_cls"])
    named = dict(m.named_parameters())
    for k in _watched(cfg, c):
        g, r = named[k].grad.cpu(), G[k]
        if k.endswith("word_embeddings.weight"):
            rows = torch.unique(c["ids"][c["ids"] != cfg.pad_id])
            assert rows.numel() > 8
            rest = torch.ones(cfg.vocab, dtype=torch.bool)
            rest[rows] = False
            assert (g[rest] == 0).all()                  # rows that do not occur (and the padding row) get exactly nothing
            g, r = g[rows], r[rows]
        if k.endswith("token_type_embeddings.weight") and kind == "bert":
            assert r.norm(dim=1).min() > 0               # both rows of BERT's type table are exercised
        err = (g - r).norm().item() / r.norm().item()
        print(f"  {k}: {err:.3e}")
        assert err < TOL_GRAD[dtype], (k, err)
    for k in ("bert_model.pooler.dense.weight", "bert_model.pooler.dense.bias"):
        inf = next(i for i in m._infos if i["name"] == k)
        assert named[k].grad is None and G[k] is None
        assert (m._flat_grad[inf["offset"]: inf["offset"] + inf["numel"]] == 0).all()


def _steps(kind, dtype, fused, n, c):
    from smtc_amd.config import Config  # noqa: F401
    from smtc_amd.text_only import TextModel

    class Cfg:
        batch_size, num_labels, max_length, dropout, use_loss_correction = 8, 3, 64, 0.1, False
    cfg = c["cfg"]
    name, a = KINDS[kind]
    tm = TextModel(Cfg, name, arch=dict(a, layers=cfg.layers_txt, vocab=cfg.vocab), dtype=dtype, device=DEV, seed=3)
    tm.model.load_state_dict(c["P"], strict=False)
    losses = []
    for st in range(1, n + 1):
        f = tm.train_step if fused else tm.staged_step
        loss, ncorr = f(c["ids"], c["mask"], c["tt"], c["onehot"], c["w"], 1e-3, 0.01, st, seed=1000 + st)
        losses.append(loss.item())
    torch.cuda.synchronize()
    return tm, losses


@pytest.mark.parametrize("kind,dtype", [("xlmr", "bf16"), ("bert", "bf16x3"), ("xlmr", "f16")])
def test_fused_step_is_the_staged_step(kind, dtype, monkeypatch):
    """MMHIP_DETERMINISTIC=1: fused train_step == forward, loss, backward, AdamW as separate calls, bit for bit, over three steps; and twice the same"""
    monkeypatch.setenv("MMHIP_DETERMINISTIC", "1")
    c = _case(kind)
    a, la = _steps(kind, dtype, True, 3, c)
    b, lb = _steps(kind, dtype, False, 3, c)
    a2, la2 = _steps(kind, dtype, True, 3, c)
    assert la == lb == la2
    assert torch.equal(a.model._flat_train, b.model._flat_train) and torch.equal(a.model._flat_train, a2.model._flat_train)
    for i in range(2):
        assert torch.equal(a._opt[i], b._opt[i]) and torch.equal(a._opt[i], a2._opt[i])
    assert not torch.equal(a.model._flat_train[a.model._word_info["offset"] - 4096: a.model._word_info["offset"]],
                           torch.zeros(4096, device=DEV))


def test_capacity_growth_between_training_steps_leaves_no_trace(monkeypatch):
    """the handle is re-created WHILE TRAINING: trainer A is made at capacity (2, 16) and meets a (4, 32) batch in its second step, trainer B is made
    at (4, 32).  Same seed, weights and steps, MMHIP_DETERMINISTIC=1: parameters, both moments, the row flags and the losses are bit-identical.
    Then a token id == vocab on the grown handle reaches check_indices(): the index counter was attached to the new handle too."""
    from smtc_amd.text_only import TextModel
    monkeypatch.setenv("MMHIP_DETERMINISTIC", "1")
    batches = [_case("xlmr", 2, 16, 8), _case("xlmr")]
    cfg = batches[1]["cfg"]
    name, a = KINDS["xlmr"]
    res, trainers = [], []
    for cap_b, cap_t in ((2, 16), (4, 32)):
        class Cfg:
            batch_size, num_labels, max_length, dropout, use_loss_correction = cap_b, 3, cap_t, 0.1, False
        tm = TextModel(Cfg, name, arch=dict(a, layers=2, vocab=500), dtype="bf16", device=DEV, seed=3)
        tm.model.load_state_dict(batches[1]["P"], strict=False)
        assert cfg.layers_txt == 2 and cfg.vocab == 500 and tm.model._capacity == (cap_b, cap_t)
        losses = []
        for st, c in enumerate(batches, 1):
            loss, _ = tm.train_step(c["ids"], c["mask"], c["tt"], c["onehot"], c["w"], 1e-3, 0.01, st)
            losses.append(loss.clone())
        torch.cuda.synchronize()
        assert tm.model._capacity == (4, 32)
        res.append((tm.model._flat_train.clone(), tm._opt[0].clone(), tm._opt[1].clone(), tm.model._word_row_state.clone(), torch.cat(losses).cpu()))
        trainers.append(tm)
    for what, x, y in zip(("flat_train", "adam_m", "adam_v", "row_state", "losses"), res[0], res[1]):
        assert torch.equal(x, y), (what, (x.float() - y.float()).abs().max().item())
    assert res[0][0].isfinite().all() and float(res[0][4][-1]) > 0 and int(res[0][3].sum()) > 0
    tm, c = trainers[0], batches[1]
    tm.check_indices()
    bad = c["ids"].clone()
    bad[1, 2] = 500
    tm.train_step(bad, c["mask"], c["tt"], c["onehot"], c["w"], 1e-3, 0.01, 3)
    with pytest.raises(IndexError):
        tm.check_indices()


@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_training_steps(kind):
    """eight fused steps on one batch: finite, decreasing loss; the pooler bit-unchanged; the gradient buffer cleared"""
    c = _case(kind)
    from smtc_amd.text_only import TextModel

    class Cfg:
        batch_size, num_labels, max_length, dropout, use_loss_correction = 8, 3, 64, 0.0, False
    cfg = c["cfg"]
    name, a = KINDS[kind]
    tm = TextModel(Cfg, name, arch=dict(a, layers=cfg.layers_txt, vocab=cfg.vocab, p_hidden=0.0, p_attn=0.0), dtype="bf16", device=DEV, seed=3)
    tm.model.load_state_dict(c["P"], strict=False)
    losses = [tm.train_step(c["ids"], c["mask"], c["tt"], c["onehot"], c["w"], 1e-4, 0.01, st)[0].item() for st in range(1, 9)]
    print("losses", losses)
    assert all(math.isfinite(x) for x in losses) and losses[-1] < losses[0] and min(losses[4:]) < min(losses[:2])
    sd = tm.model.state_dict()
    for k in ("bert_model.pooler.dense.weight", "bert_model.pooler.dense.bias"):
        assert torch.equal(sd[k].cpu(), c["P"][k])
    assert not torch.equal(sd["linear.weight"].cpu(), c["P"]["linear.weight"])
    assert (tm.model._flat_grad == 0).all()
    r = tm.eval([{"ids": c["ids"], "mask": c["mask"], "token_type_ids": c["tt"] if c["tt"] is not None else torch.zeros_like(c["ids"]),
                  "target": c["onehot"], "data_id": torch.arange(4)}], class_weight=c["w"])
    assert set(r) == {"data_id", "loss", "predictions", "labels"} and math.isfinite(r["loss"]) and r["predictions"].shape == (4,)


def test_eval_is_the_forward_and_loss_calls_over_the_loader(capsys):
    """TextModel.eval over two loader items (3 and 2 posts of 8 tokens, padded rows, BERT token types; 1 layer, hidden 128, 2 heads) against what
    this test computes from _engine_forward and mmhip_txt_loss on the same items: the loss as the same float computation (the mean of the batch
    losses, not of the posts), predictions, labels, data ids, the printed line; and the evaluation ends with the clamped-index check"""
    from smtc_amd.text_only import TextModel

    class Cfg:
        batch_size, num_labels, max_length, dropout, use_loss_correction = 3, 3, 8, 0.1, False
    name, a = KINDS["bert"]
    tm = TextModel(Cfg, name, arch=dict(a, layers=1, hidden=128, heads=2, inter=256, vocab=50), dtype="bf16", device=DEV, seed=3)
    m, lib = tm.model, _lib.lib()
    assert m._capacity == (3, 8)
    g, items = torch.Generator().manual_seed(11), []
    for n, first in ((3, 0), (2, 3)):
        mask = torch.ones(n, 8, dtype=torch.int64)
        mask[n - 1, 5:] = 0
        ids = torch.randint(1, 50, (n, 8), generator=g) * mask
        tt = (torch.arange(8).expand(n, 8) >= 3).long() * mask
        items.append({"ids": ids, "mask": mask, "token_type_ids": tt, "target": torch.eye(3, dtype=torch.int64)[torch.randint(0, 3, (n,), generator=g)],
                      "data_id": torch.arange(first, first + n)})
    w = torch.tensor([1.0, 2.0, 0.5])
    cw = w.to(DEV)
    m.eval()
    losses, accs, preds, labels = [], [], [], []
    with torch.no_grad():
        for it in items:
            out = m._engine_forward(*tm._batch(it))
            onehot, loss = it["target"].to(DEV), torch.empty(1, device=DEV)
            _lib.check(lib.mmhip_txt_loss(m._handle, _lib.ptr(onehot), _lib.ptr(cw), _lib.ptr(loss), None, _lib.stream_ptr()), "txt_loss")
            losses.append(loss)
            preds.append(out.argmax(dim=1).cpu())
            labels.append(it["target"].argmax(dim=1))
            accs.append((preds[-1] == labels[-1]).float().mean().reshape(1) * 100)
    want_loss, want_acc = float(torch.cat(losses).mean().item()), float(torch.cat(accs).mean().item())
    assert math.isfinite(want_loss) and losses[0].item() != losses[1].item()
    capsys.readouterr()
    r = tm.eval(items, class_weight=w)
    assert capsys.readouterr().out == f"loss: {want_loss:.4f} acc: {want_acc:.4f}\n\n"
    assert list(r) == ["data_id", "loss", "predictions", "labels"] and type(r["loss"]) is float and r["loss"] == want_loss
    for k, want in (("predictions", torch.cat(preds)), ("labels", torch.cat(labels)), ("data_id", torch.arange(5))):
        assert r[k].dtype == np.int64 and r[k].tolist() == want.tolist(), k
    assert not m.training and set(m._last) == {"B", "T", "seed", "ids"} and (m._last["B"], m._last["T"]) == (2, 8)
    bad = dict(items[1], ids=items[1]["ids"].clone())
    bad["ids"][0, 1] = 50                                   # == vocab: clamped into the word table by the engine, counted
    with pytest.raises(IndexError, match="1 token id"):
        tm.eval([bad], class_weight=w)


@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_trimmed_batch_gives_the_padded_logits(kind):
    """T = 64 with every post shorter than 32 tokens: the batch trimmed to its longest post gives the padded batch's logits"""
    c = _case(kind)
    cfg = c["cfg"]
    pad = lambda x, v: torch.cat([x, torch.full((x.shape[0], 32), v, dtype=x.dtype)], dim=1)
    ids, mask = pad(c["ids"], cfg.pad_id), pad(c["mask"], 0)
    tt = None if c["tt"] is None else pad(c["tt"], 0)
    m = _model(kind, "bf16x3", c)
    m.eval()
    with torch.no_grad():
        full = (m(ids, mask) if kind == "xlmr" else m(ids, mask, tt)).cpu()
        short = _call(m, c, kind).cpu()
    ref = _ref_eval(c)
    assert (full - short).abs().max().item() <= 1e-5 * ref.abs().max().item()
    assert (full - ref).abs().max().item() / ref.abs().max().item() < TOL_OUT["bf16x3"]["out_cls"]


@pytest.mark.parametrize("kind", ["xlmr", "bert"])
def test_trainer_batch_trims_a_loader_item(kind):
    """TextModel._batch on a loader item padded to T = 64 (the dataset's keys; BERT: non-zero token types): ids, mask and token types leave trimmed
    to the 32 columns in use, on the device, under the names the model takes -- and give the padded item's logits"""
    from smtc_amd.text_only import TextModel
    c = _case(kind)
    cfg = c["cfg"]

    class Cfg:
        batch_size, num_labels, max_length, dropout, use_loss_correction = 8, 3, 64, 0.0, False
    name, a = KINDS[kind]
    tm = TextModel(Cfg, name, arch=dict(a, layers=cfg.layers_txt, vocab=cfg.vocab, p_hidden=0.0, p_attn=0.0), dtype="bf16x3", device=DEV, seed=3)
    tm.model.load_state_dict(c["P"], strict=False)
    pad = lambda x, v: torch.cat([x, torch.full((x.shape[0], 32), v, dtype=x.dtype)], dim=1)
    item = {"ids": pad(c["ids"], cfg.pad_id), "mask": pad(c["mask"], 0), "target": c["onehot"], "data_id": torch.arange(4)}
    if kind == "bert":
        item["token_type_ids"] = pad(c["tt"], 0)
    ids, mask, tt = tm._batch(item)
    assert ids.is_cuda and mask.is_cuda and tuple(ids.shape) == tuple(mask.shape) == (4, 32)
    assert torch.equal(ids.cpu(), c["ids"]) and torch.equal(mask.cpu(), c["mask"])
    if kind == "bert":
        assert tt.is_cuda and torch.equal(tt.cpu(), c["tt"]) and int(tt.sum()) > 0
    else:
        assert tt is None
    m = tm.model
    m.eval()
    with torch.no_grad():
        short = (m(ids, mask) if kind == "xlmr" else m(ids, mask, tt)).cpu()
        full = (m(item["ids"], item["mask"]) if kind == "xlmr" else m(item["ids"], item["mask"], item["token_type_ids"])).cpu()
    ref = _ref_eval(c)
    assert (full - short).abs().max().item() <= 1e-5 * ref.abs().max().item()
    assert (short - ref).abs().max().item() / ref.abs().max().item() < TOL_OUT["bf16x3"]["out_cls"]


def test_late_fusion_calls_refuse_a_text_only_handle():
    """include/mmhip.h: the late-fusion calls that name the image tower or ITC answer an error for a text-only handle instead of touching memory"""
    c = _case("xlmr")
    m = _model("xlmr", "bf16", c)
    m.eval()
    with torch.no_grad():
        _call(m, c, "xlmr")
    lib, s = _lib.lib(), _lib.stream_ptr()
    assert lib.mmhip_refresh_weights(m._handle, 1, s) != 0 and lib.mmhip_refresh_weights(m._handle, 3, s) != 0
    assert lib.mmhip_set_itc_global(m._handle, 1, 0) != 0 and lib.mmhip_reserve_itc_global(m._handle, 2) != 0
    assert lib.mmhip_txt_refresh_weights(m._handle, s) == 0
    torch.cuda.synchronize()


def test_cls_only_off_restores_the_full_last_layer(monkeypatch):
    """MMHIP_CLS_ONLY=0: the last layer runs on every row; logits and gradients agree with the CLS-only default within the parity bound"""
    c = _case("xlmr")
    outs = []
    for v in ("1", "0"):
        monkeypatch.setenv("MMHIP_CLS_ONLY", v)
        m = _model("xlmr", "bf16x3", c, dropout=0.0)
        m.train()
        logits = _call(m, c, "xlmr")
        O.cls_loss(logits, c["onehot"].to(DEV), c["w"].to(DEV)).backward()
        named = dict(m.named_parameters())
        outs.append((logits.detach().cpu(), named["bert_model.encoder.layer.0.attention.self.query.weight"].grad.cpu(), named["linear.weight"].grad.cpu()))
    for a, b in zip(*outs):
        assert (a - b).norm().item() <= 1e-3 * b.norm().item()


def test_checkpoint_keys_and_cli(tmp_path):
    """python -m smtc_amd.run_txt --model_name bernice --task 3 --synthetic --epochs 1 in a fresh process: exit 0, a finite loss; the checkpoint it
    saves has exactly the reference module's keys and shapes"""
    cmd = [sys.executable, "-m", "smtc_amd.run_txt", "--model_name", "bernice", "--task", "3", "--synthetic", "--epochs", "1", "--arch_layers", "2",
           "--n_synthetic", "48", "--save_model", "--results_dir", str(tmp_path) + "/"]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    vals = [float(l.rsplit("loss", 1)[1]) for l in r.stdout.splitlines() if l.startswith("Got ") and "loss" in l]
    assert vals and all(math.isfinite(v) for v in vals), r.stdout[-2000:]
    sd = torch.load(os.path.join(str(tmp_path), "bernice_task3_seed30_net.pth"), map_location="cpu")
    from smtc_amd.config import TEXT_ARCH
    a = TEXT_ARCH["bernice"]
    want = R.param_shapes(R.oracle_cfg(layers=2, vocab=a["vocab"], num_labels=3, kind="xlmr"))
    want["bert_model.embeddings.position_ids"] = (1, a["max_pos"])
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
