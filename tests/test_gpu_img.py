"""Image-only path on the GPU: the ViT embedding backward against fp64 with per-element bounds, the ViTClassifier drop-in against the fp32 restatement
of the reference model (tests/img_ref.py) and the reference's own golden, the fused step against the staged one, the command line.

Shapes: 2 layers, hidden 768, 3 labels, class weights [1, 2, 0.5]; 192 px (145 tokens: 5 attention tiles -> 3 + 2, last tile 17 rows) with B = 2 and
224 px (197 tokens: 7 tiles -> 4 + 3, last tile 5 rows) with B = 3 -- the two ways the long attention backward chunks its keys.
Tolerances of the model tests are the ones tests/test_gpu_model.py holds the late-fusion model to (imported, not restated)."""
import json
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
import img_ref as R
from test_gpu_model import TOL_OUT, TOL_GRAD, TOL_LOSS, TOL_GRAD_BWD_PRODUCTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SHAPES = [(192, 2), (224, 3)]
DTYPES = ["bf16x3", "bf16", "f16"]

# ------------------------------------------------------------------------------------------------ mmhip_op_vit_embed_bwd
SPLIT_POSTS = 8          # csrc/mmhip_kernels.h VIT_EMBED_BWD_POSTS: more posts than this are cut into slices whose partial rows a second launch sums
GUARD = 64               # elements of sentinel either side of every output
OPDT = {"bf16": (_lib.BF16, torch.bfloat16), "f16": (_lib.F16, torch.float16), "f32": (_lib.F32, torch.float32), "pair": (_lib.PAIR, torch.float32)}


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD: GUARD + n]


def _embed_bwd(name, B, P, H, alpha, hi_only=0, seed=0):
    """one call on guarded buffers -> everything a check needs.  Bound of the sums, per element, from the kernel's rounding points: the posts are added
    one after the other in fp32 (slices of 8 first, then the slices: never more than B - 1 additions on one path), the sum is multiplied by alpha and
    added to what dpos / dcls held -- B roundings relative to alpha * sum_b |dx| (gamma_B = B u / (1 - B u)), one more on the stored result."""
    lib, s = _lib.lib(), _lib.stream_ptr()
    code, td = OPDT[name]
    alpha = float(np.float32(alpha))          # the entry point takes a C float: the reference uses the value the kernel receives
    g = torch.Generator().manual_seed(seed)
    dx = (torch.randn(B, P, H, generator=g) * torch.rand(B, P, 1, generator=g)).to(td)
    d0 = torch.randn(P, H, generator=g)
    c0 = torch.randn(H, generator=g)
    dxg = dx.to(DEV)
    fill_out = 7.0
    dposb, dpos = _guarded(P * H, torch.float32, fill_out)
    dclsb, dcls = _guarded(H, torch.float32, fill_out)
    dpos.copy_(d0.flatten())
    dcls.copy_(c0)
    if name == "pair":
        dpeb, dpe = _guarded(B * (P - 1) * 2 * H, torch.bfloat16, 5.0)
    else:
        dpeb, dpe = _guarded(B * (P - 1) * H, td, 5.0)
    need = lib.mmhip_op_vit_embed_bwd_ws_bytes(B, P, H)
    assert (need > 0) == (B > SPLIT_POSTS)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    rc = lib.mmhip_op_vit_embed_bwd(code, _lib.ptr(dxg), B, P, H, alpha, _lib.ptr(dpos), _lib.ptr(dcls), _lib.ptr(dpe), hi_only, _lib.ptr(ws), need, s)
    assert rc == 0, rc
    torch.cuda.synchronize()
    x64 = dx.double()
    S = x64.abs().sum(dim=0)
    u = B * OB.U_32 / (1 - B * OB.U_32)
    ref_pos = d0.double() + alpha * x64.sum(dim=0)
    b_pos = abs(alpha) * u * S + OB.U_32 * (d0.double().abs() + abs(alpha) * S) + 1e-30
    ref_cls = c0.double() + alpha * x64[:, 0].sum(dim=0)
    b_cls = abs(alpha) * u * S[0] + OB.U_32 * (c0.double().abs() + abs(alpha) * S[0]) + 1e-30
    return dict(dx=dx, dposb=dposb, dclsb=dclsb, dpeb=dpeb, dpos=dpos, dcls=dcls, dpe=dpe, ref_pos=ref_pos, b_pos=b_pos, ref_cls=ref_cls, b_cls=b_cls,
                fill_out=fill_out)


def _guards_intact(r, tag):
    for buf, fill in ((r["dposb"], r["fill_out"]), (r["dclsb"], r["fill_out"]), (r["dpeb"], 5.0)):
        assert (buf[:GUARD].float() == fill).all() and (buf[-GUARD:].float() == fill).all(), tag


@pytest.mark.parametrize("name", ["bf16", "f16", "f32", "pair"])
def test_vit_embed_bwd_per_element(name):
    """P in {145, 197} x B in {1, 3, 9} (9 > SPLIT_POSTS = 8: the split-B path, two slices of 8 + 1 posts), H = 768, alpha != 1, accumulation onto
    non-zero dpos / dcls, guard bands: every sum within its bound, the compact copy bit-equal (pairs: hi is a nearest bf16 and hi + lo within the
    pair's 2^-16), two calls equal bits"""
    H = 768
    for P in (145, 197):
        for B in (1, 3, SPLIT_POSTS + 1):
            for alpha in (0.37, 1.0 / 1024):
                tag = (name, P, B, alpha)
                r = _embed_bwd(name, B, P, H, alpha)
                got = r["dpos"].view(P, H).cpu().double()
                assert ((got - r["ref_pos"]).abs() <= r["b_pos"]).all(), (tag, ((got - r["ref_pos"]).abs() / r["b_pos"]).max().item())
                gc = r["dcls"].cpu().double()
                assert ((gc - r["ref_cls"]).abs() <= r["b_cls"]).all(), tag
                patches = r["dx"][:, 1:].reshape(B * (P - 1), H)
                if name == "pair":
                    pe = r["dpe"].view(B * (P - 1), 2 * H).cpu()
                    hi, lo = pe[:, :H], pe[:, H:]
                    assert OB.pair_hi_is_nearest(hi, lo).all(), tag
                    assert ((hi.double() + lo.double() - patches.double()).abs() <= OB.U_PAIR * patches.double().abs()).all(), tag
                else:
                    view = torch.int32 if name == "f32" else torch.int16
                    assert torch.equal(r["dpe"].view(B * (P - 1), H).cpu().view(view), patches.contiguous().view(view)), tag
                _guards_intact(r, tag)
                r2 = _embed_bwd(name, B, P, H, alpha)
                assert torch.equal(r["dposb"], r2["dposb"]) and torch.equal(r["dclsb"], r2["dclsb"]) and torch.equal(r["dpeb"], r2["dpeb"]), tag
    # the one-product form of the pair: the hi plane alone, the lo plane's words keep what they held
    r = _embed_bwd("pair", 3, 145, H, 0.37, hi_only=1)
    pe = r["dpe"].view(3 * 144, 2 * H).cpu()
    assert torch.equal(pe[:, :H], r["dx"][:, 1:].reshape(3 * 144, H).to(torch.bfloat16)) and (pe[:, H:].float() == 5.0).all()
    _guards_intact(r, "hi_only")


def test_vit_embed_bwd_rejects_misaligned_pointers():
    """16-byte accesses throughout: a pointer 8 bytes off is MMHIP_E_INVALID before any launch, nothing written"""
    lib, s, B, P, H = _lib.lib(), _lib.stream_ptr(), 2, 145, 768
    dx = torch.ones(B * P * H + 8, dtype=torch.bfloat16, device=DEV)
    dpos = torch.full((P * H + 8,), 3.0, device=DEV)
    dcls = torch.full((H + 8,), 3.0, device=DEV)
    dpe = torch.full((B * (P - 1) * H + 8,), 3.0, dtype=torch.bfloat16, device=DEV)
    off = lambda t, n: _lib.ptr(t[n:])
    f = lambda a=0, b=0, c=0, d=0: lib.mmhip_op_vit_embed_bwd(_lib.BF16, off(dx, a), B, P, H, 1.0, off(dpos, b), off(dcls, c), off(dpe, d), 0, None, 0, s)
    assert f(a=4) == -1 and f(b=2) == -1 and f(c=2) == -1 and f(d=4) == -1
    torch.cuda.synchronize()
    assert (dpos == 3.0).all() and (dcls == 3.0).all() and (dpe.float() == 3.0).all()
    assert f() == 0 and f(a=8, b=4, c=4, d=8) == 0          # 16-byte offsets are fine
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the model
_REF = {}
W = torch.tensor([1.0, 2.0, 0.5])


def _case(image, B, seed_p=0):
    """inputs, weights and class weights -- computed once, shared, never changed; the restatement's results are added lazily"""
    key = (image, B, seed_p)
    if key not in _REF:
        cfg = R.oracle_cfg(image=image)
        _, px, onehot = R.pixels_u8(cfg, B, 7)
        _REF[key] = dict(cfg=cfg, px=px, onehot=onehot, w=W, P=R.make_params(cfg, seed_p), image=image, B=B)
    return _REF[key]


def _ref_eval(c):
    if "eval" not in c:
        with torch.no_grad():
            c["eval"] = R.forward(c["P"], c["px"], c["cfg"])
    return c["eval"]


def _ref_grads(c):
    if "grads" not in c:
        c["grads"] = R.loss_and_grads(c["P"], c["px"], c["onehot"], c["w"], c["cfg"])
    return c["grads"]


def _model(dtype, c, max_posts=None, **kw):
    from smtc_amd.image_only import ViTClassifier
    cfg = c["cfg"]
    m = ViTClassifier("", cfg.num_labels, arch=dict(layers=cfg.layers_img, image=c["image"]), dtype=dtype, max_posts=max_posts or c["B"], device=DEV, **kw)
    sd = m.state_dict()
    assert set(sd) == set(c["P"]) and all(tuple(sd[k].shape) == tuple(v.shape) for k, v in c["P"].items())
    m.load_state_dict(c["P"])
    return m


def _watched(cfg):
    """both layers: query weight / bias, value weight, attention-output weight, layernorm_before.weight, layernorm_after.bias, both MLP weights, one MLP
    bias; every embedding parameter; vit.layernorm.*; classifier.*.  (Key biases are left out: their gradient is rounding residue around zero.)"""
    w = ["classifier.weight", "classifier.bias", "vit.layernorm.weight", "vit.layernorm.bias", "vit.embeddings.cls_token",
         "vit.embeddings.position_embeddings", "vit.embeddings.patch_embeddings.projection.weight", "vit.embeddings.patch_embeddings.projection.bias"]
    for l in range(cfg.layers_img):
        p = f"vit.encoder.layer.{l}."
        w += [p + n for n in ("attention.attention.query.weight", "attention.attention.query.bias", "attention.attention.value.weight",
                              "attention.output.dense.weight", "layernorm_before.weight", "layernorm_after.bias", "intermediate.dense.weight",
                              "intermediate.dense.bias", "output.dense.weight")]
    return w


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("image,B", SHAPES)
def test_eval_logits(image, B, dtype):
    """against the restatement and, at 192 px, against the logits the reference's own ViTForImageClassification computed (the golden)"""
    c = _case(image, B)
    m = _model(dtype, c)
    m.eval()
    with torch.no_grad():
        out = m(c["px"]).logits.cpu()
    ref = _ref_eval(c)
    err = (out - ref).abs().max().item() / ref.abs().max().item()
    print(f"eval logits {image} {dtype}: {err:.3e}")
    assert err < TOL_OUT[dtype]["out_cls"]
    if image == 192:
        z = np.load(os.path.join(ROOT, "tests", "golden", "img_small_vit.npz"), allow_pickle=False)
        assert torch.equal(R.from_u8(torch.from_numpy(z["pixels_u8"])), c["px"])
        gold = torch.from_numpy(z["logits"])
        e2 = (out - gold).abs().max().item() / gold.abs().max().item()
        print(f"eval logits vs reference golden {dtype}: {e2:.3e}")
        assert e2 < TOL_OUT[dtype]["out_cls"]


def _backward(m, c):
    m.train()
    logits = m(c["px"]).logits
    loss = O.cls_loss(logits, c["onehot"].to(DEV), c["w"].to(DEV))
    loss.backward()
    return logits.detach().cpu(), loss.item(), {k: v.grad.cpu() for k, v in m.named_parameters()}


def _check_grads(c, g, tol, tag):
    _, _, G = _ref_grads(c)
    errs = {}
    for k in _watched(c["cfg"]):
        errs[k] = (g[k] - G[k]).norm().item() / G[k].norm().item()
        print(f"  {tag} {k}: {errs[k]:.3e}")
    bad = {k: e for k, e in errs.items() if not e < tol}
    assert not bad, (tag, bad)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("image,B", SHAPES)
def test_loss_and_gradients(image, B, dtype):
    """loss.backward() on the returned logits: loss and per-tensor relative L2 on the watch list; parity mode at 1e-3 is the gate on the logic"""
    c = _case(image, B)
    m = _model(dtype, c)
    logits, loss, g = _backward(m, c)
    r_logits, r_loss, _ = _ref_grads(c)
    e_loss = abs(loss - r_loss.item()) / abs(r_loss.item())
    print(f"train loss {image} {dtype}: {loss:.6f} vs {r_loss.item():.6f} ({e_loss:.2e})")
    assert e_loss < (TOL_LOSS[dtype] if dtype == "bf16x3" else TOL_OUT[dtype]["out_cls"])
    _check_grads(c, g, TOL_GRAD[dtype], f"{image} {dtype}")
    # a key bias's gradient is zero in exact arithmetic: residue far below the same layer's query-bias gradient (parity mode; 16-bit noise is larger)
    if dtype == "bf16x3":
        for l in range(c["cfg"].layers_img):
            p = f"vit.encoder.layer.{l}.attention.attention."
            assert g[p + "key.bias"].abs().max() < 1e-3 * g[p + "query.bias"].abs().max()


@pytest.mark.parametrize("products", [3, 2, 1])
@pytest.mark.parametrize("image,B", SHAPES)
def test_backward_products(image, B, products):
    """mmhip_set_backward_products in parity mode: the forward keeps three products (logits and loss at bf16x3's bounds), every watched gradient within
    the project's bound for the policy"""
    c = _case(image, B)
    m = _model("bf16x3", c, backward_products=products)
    logits, loss, g = _backward(m, c)
    r_logits, r_loss, _ = _ref_grads(c)
    assert (logits - r_logits).abs().max().item() / r_logits.abs().max().item() < TOL_OUT["bf16x3"]["out_cls"]
    assert abs(loss - r_loss.item()) / abs(r_loss.item()) < TOL_LOSS["bf16x3"]
    _check_grads(c, g, TOL_GRAD_BWD_PRODUCTS[products], f"{image} products={products}")


def _trainer(dtype, c, max_posts=None):
    from smtc_amd.image_only import ImageModel
    tm = ImageModel(max_posts or c["B"], 3, "vit", arch=dict(layers=c["cfg"].layers_img, image=c["image"]), dtype=dtype, device=DEV, seed=3)
    tm.model.load_state_dict(c["P"])
    return tm


def _steps(dtype, fused, n, c, lr=1e-3, wd=0.01):
    tm = _trainer(dtype, c)
    losses = []
    for st in range(1, n + 1):
        loss, _ = (tm.train_step if fused else tm.staged_step)(c["px"], c["onehot"], c["w"], lr, wd, st)
        losses.append(loss.item())
    torch.cuda.synchronize()
    return tm, losses


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("image,B", SHAPES)
def test_fused_step_is_the_staged_step(image, B, dtype, monkeypatch):
    """MMHIP_DETERMINISTIC=1: fused train_step == forward, loss, backward, AdamW as separate calls, bit for bit, over three steps; and twice the same"""
    monkeypatch.setenv("MMHIP_DETERMINISTIC", "1")
    c = _case(image, B)
    a, la = _steps(dtype, True, 3, c)
    b, lb = _steps(dtype, False, 3, c)
    a2, la2 = _steps(dtype, True, 3, c)
    assert la == lb == la2 and all(math.isfinite(x) for x in la)
    assert torch.equal(a.model._flat_train, b.model._flat_train) and torch.equal(a.model._flat_train, a2.model._flat_train)
    for i in range(2):
        assert torch.equal(a._opt[i], b._opt[i]) and torch.equal(a._opt[i], a2._opt[i])
    assert (a.model._flat_grad == 0).all()
    sd = a.model.state_dict()
    moved = [k for k in c["P"] if not torch.equal(sd[k].cpu(), c["P"][k])]
    assert len(moved) == len(c["P"])          # every parameter is stepped (one AdamW group; a key bias moves by its residue's sign)


@pytest.mark.parametrize("image,B", SHAPES)
def test_three_training_steps_track_the_restatement(image, B):
    """three fused steps in parity mode against img_ref + O.adamw_step: the loss of the first step, taken on the same parameters, at TOL_LOSS; the
    losses of the second and third, taken on parameters that already carry the update's error below, at the band of the logits they are computed
    from, TOL_OUT['bf16x3']['out_cls'], as are the eval logits after the last; and the three-step UPDATE of every watched tensor.
    Bound of the update (the issue names none; this one is an estimate, not a proof): Adam's early steps are sign-like (lr g / (|g| + eps)); an
    element whose gradient lies within the gradient's error of zero may take the opposite step, 2 lr off.  With a gradient error of eps_g relative to
    the tensor's rms, and ASSUMING the gradient's elements are spread like a bell curve around zero (density 1 / (sqrt(2 pi) rms) = 0.4 / rms there),
    a fraction of about 0.8 eps_g of them lies that close to zero, so the update's relative L2 error is about 2 sqrt(0.8 eps_g); with
    eps_g = TOL_GRAD['bf16x3'] and the 0.8 rounded up to 1, 2 sqrt(TOL_GRAD) = 6.3e-2.  A tensor whose gradient is far from that shape (mass piled
    at zero) could need more; none of the watched ones is held to anything else."""
    c = _case(image, B)
    cfg, lr, wd = c["cfg"], 1e-3, 0.01
    if "traj" not in c:
        P = {k: v.clone() for k, v in c["P"].items()}
        M = {k: torch.zeros_like(v) for k, v in P.items()}
        V = {k: torch.zeros_like(v) for k, v in P.items()}
        losses = []
        for st in range(1, 4):
            _, loss, G = R.loss_and_grads(P, c["px"], c["onehot"], c["w"], cfg)
            losses.append(loss.item())
            R.adamw(P, G, M, V, st, lr, wd)
        with torch.no_grad():
            c["traj"] = (losses, P, R.forward(P, c["px"], cfg))
    r_losses, r_P, r_logits = c["traj"]
    tm, losses = _steps("bf16x3", True, 3, c, lr, wd)
    for st, (a, b) in enumerate(zip(losses, r_losses)):
        print(f"step loss {a:.6f} vs {b:.6f}")
        assert abs(a - b) / abs(b) < (TOL_LOSS["bf16x3"] if st == 0 else TOL_OUT["bf16x3"]["out_cls"])
    tm.model.eval()
    with torch.no_grad():
        out = tm.model(c["px"]).logits.cpu()
    assert (out - r_logits).abs().max().item() / r_logits.abs().max().item() < TOL_OUT["bf16x3"]["out_cls"]
    sd = tm.model.state_dict()
    bound = 2 * math.sqrt(TOL_GRAD["bf16x3"])
    for k in _watched(cfg):
        du, dr = sd[k].cpu() - c["P"][k], r_P[k] - c["P"][k]
        err = (du - dr).norm().item() / dr.norm().item()
        print(f"  update {k}: {err:.3e}")
        assert err < bound, (k, err)


def test_capacity_growth_between_training_steps_leaves_no_trace(monkeypatch):
    """the handle is re-created WHILE TRAINING: trainer A is made for 2 posts and meets 3 in its second step, trainer B is made for 3.  Same weights
    and steps, MMHIP_DETERMINISTIC=1: parameters, both moments and the losses are bit-identical"""
    monkeypatch.setenv("MMHIP_DETERMINISTIC", "1")
    batches = [_case(192, 2), _case(192, 3)]
    res = []
    for cap in (2, 3):
        tm = _trainer("bf16", batches[0], max_posts=cap)
        assert tm.model._capacity == (cap,)
        losses = [tm.train_step(c["px"], c["onehot"], c["w"], 1e-3, 0.01, st)[0].clone() for st, c in enumerate(batches, 1)]
        torch.cuda.synchronize()
        assert tm.model._capacity == (3,)
        res.append((tm.model._flat_train.clone(), tm._opt[0].clone(), tm._opt[1].clone(), torch.cat(losses).cpu()))
    for what, x, y in zip(("flat_train", "adam_m", "adam_v", "losses"), res[0], res[1]):
        assert torch.equal(x, y), (what, (x.float() - y.float()).abs().max().item())
    assert res[0][0].isfinite().all() and float(res[0][3][-1]) > 0


def test_eval_is_the_forward_and_loss_calls_over_the_loader(capsys):
    """ImageModel.eval over two loader items (2 images and 1 image of 192 px, as the dataset hands them: [n, 1, 3, S, S]; 1 layer, hidden 128,
    2 heads) against what this test computes from _engine_forward and mmhip_img_loss on the same items: the loss as the same float computation
    (the mean of the batch losses, not of the images), predictions, labels, data ids, the printed line"""
    from smtc_amd.image_only import ImageModel
    tm = ImageModel(2, 3, "vit", arch=dict(layers=1, hidden=128, heads=2, inter=256, image=192), dtype="bf16", device=DEV, seed=3)
    m, lib = tm.model, _lib.lib()
    assert m._capacity == (2,)
    g, items = torch.Generator().manual_seed(11), []
    for n, first in ((2, 0), (1, 2)):
        items.append({"pixel_values": torch.rand(n, 1, 3, 192, 192, generator=g) * 2 - 1, "data_id": torch.arange(first, first + n),
                      "labels": torch.eye(3, dtype=torch.int64)[torch.randint(0, 3, (n,), generator=g)]})
    cw = W.to(DEV)
    m.eval()
    losses, accs, preds, labels = [], [], [], []
    with torch.no_grad():
        for it in items:
            out = m._engine_forward(it["pixel_values"])
            onehot, loss = it["labels"].to(DEV), torch.empty(1, device=DEV)
            _lib.check(lib.mmhip_img_loss(m._handle, _lib.ptr(onehot), _lib.ptr(cw), _lib.ptr(loss), None, _lib.stream_ptr()), "img_loss")
            losses.append(loss)
            preds.append(out.argmax(dim=1).cpu())
            labels.append(it["labels"].argmax(dim=1))
            accs.append((preds[-1] == labels[-1]).float().mean().reshape(1) * 100)
    want_loss, want_acc = float(torch.cat(losses).mean().item()), float(torch.cat(accs).mean().item())
    assert math.isfinite(want_loss) and losses[0].item() != losses[1].item()
    capsys.readouterr()
    r = tm.eval(items, class_weight=W)
    assert capsys.readouterr().out == f"test loss: {want_loss:.4f} test acc: {want_acc:.4f}\n\n"
    assert list(r) == ["data_id", "loss", "predictions", "labels"] and type(r["loss"]) is float and r["loss"] == want_loss
    for k, want in (("predictions", torch.cat(preds)), ("labels", torch.cat(labels)), ("data_id", torch.arange(3))):
        assert r[k].dtype == np.int64 and r[k].tolist() == want.tolist(), k
    assert not m.training and m._last == {"B": 1}
    empty = tm.eval([], class_weight=W)
    assert math.isnan(empty["loss"]) and all(empty[k].dtype == np.int64 and empty[k].shape == (0,) for k in ("data_id", "predictions", "labels"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_hf_directory_loads(dtype, tmp_path):
    """a directory written by the installed transformers (its own key generation) loads -- every parameter -- and the eval logits agree with that model;
    a directory under the 4.25.1 keys gives the same parameters"""
    from safetensors.torch import save_file
    from transformers import ViTConfig, ViTForImageClassification
    from smtc_amd.image_only import ViTClassifier
    from smtc_amd.mm_late import _vit_key_to_ref
    torch.manual_seed(5)
    hf = ViTForImageClassification(ViTConfig(num_hidden_layers=2, image_size=192, num_labels=3))
    with torch.no_grad():
        for n, p in hf.named_parameters():          # biases and LayerNorm weights off their initial 0 / 1, so that a missed tensor shows
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p))
    hf.eval()
    d = str(tmp_path / "hf")
    hf.save_pretrained(d)
    m = ViTClassifier(d, 3, dtype=dtype, max_posts=2, device=DEV, seed=11)
    assert m.arch["layers"] == 2 and m.arch["image"] == 192
    want = {("classifier." + k[len("classifier."):] if k.startswith("classifier.") else "vit." + _vit_key_to_ref(k[4:])): v for k, v in hf.state_dict().items()}
    sd = m.state_dict()
    assert set(sd) == set(want) and all(torch.equal(sd[k].cpu(), want[k]) for k in want)
    c = _case(192, 2)
    with torch.no_grad():
        ref = hf(pixel_values=c["px"]).logits
        m.eval()
        out = m(c["px"]).logits.cpu()
    err = (out - ref).abs().max().item() / ref.abs().max().item()
    print(f"HF directory eval logits {dtype}: {err:.3e}")
    assert err < TOL_OUT[dtype]["out_cls"]
    d2 = tmp_path / "ref_keys"
    d2.mkdir()
    save_file({k: v.contiguous() for k, v in want.items()}, str(d2 / "model.safetensors"))
    with open(os.path.join(d, "config.json")) as f, open(d2 / "config.json", "w") as g:
        json.dump(json.load(f), g)
    m2 = ViTClassifier(str(d2), 3, dtype=dtype, max_posts=2, device=DEV, seed=12)
    assert all(torch.equal(m2.state_dict()[k].cpu(), want[k]) for k in want)


def test_checkpoint_keys_and_cli(tmp_path):
    """python -m smtc_amd.run_img --model_name vit --task 3 --synthetic --epochs 1 in a fresh process: exit 0, finite losses, the reference's result
    files; the checkpoint it saves has exactly the reference model's keys (transformers 4.25.1 names) and shapes"""
    cmd = [sys.executable, "-m", "smtc_amd.run_img", "--model_name", "vit", "--task", "3", "--synthetic", "--epochs", "1", "--arch_layers", "2",
           "--n_synthetic", "32", "--batch_size", "8", "--save_model", "--save_preds", "--results_dir", str(tmp_path) + "/"]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    vals = [float(l.rsplit("loss", 1)[1]) for l in r.stdout.splitlines() if l.startswith("Got ") and "loss" in l]
    assert vals and all(math.isfinite(v) for v in vals), r.stdout[-2000:]
    for f in ("metrics_val.csv", "metrics_test.csv", "preds.csv", "net.pth"):
        assert os.path.exists(os.path.join(str(tmp_path), "vit_task3_seed30_" + f)), f
    sd = torch.load(os.path.join(str(tmp_path), "vit_task3_seed30_net.pth"), map_location="cpu")
    assert {k: tuple(v.shape) for k, v in sd.items()} == R.param_shapes(R.oracle_cfg(layers=2, image=224, num_labels=3))
