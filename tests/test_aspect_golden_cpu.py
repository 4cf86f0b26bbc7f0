"""tests/aspect_ref.py (the fp32 restatement of the reference's late-fusion model under aspect-att, and the fp64 reference of the fusion operator)
against fixtures made by the reference's own MM_Model (tests/golden/make_aspect_golden.py): forward at B = 1, 3, 4, loss and gradients without and
with ITC -- within 2e-5, the bound test_txt_golden_cpu.py holds its restatement to -- the grad-None set, and the operator's backward formulas
against torch autograd in float64."""
import ast
import os

import numpy as np
import pytest
import torch

from oracle import mm_oracle as O
import aspect_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 2e-5
TAGS = ["aspect_small_xlmr", "aspect_small_bert"]


def load(tag):
    z = np.load(os.path.join(GOLD, tag + ".npz"), allow_pickle=False)
    cfg = O.OracleConfig(**ast.literal_eval(str(z["cfg"])))
    P = O.make_params(cfg, int(z["seed_w"]))
    P[R.ASPECT_W] = P[R.ASPECT_W] * float(z["aspect_scale"])
    return z, cfg, P, (lambda k: torch.from_numpy(z[k]))


def rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("B", [1, 3, 4])
def test_forward_restatement_matches_the_reference(tag, B):
    z, cfg, P, t = load(tag)
    ids, mask = t(f"fwd{B}.ids"), t(f"fwd{B}.mask")
    assert ids.shape == (B, int(z["T"])) and (B == 1 or (mask == 0).any())          # (synthetic_batch keeps its first post at full length)
    _, _, pixels, _ = O.synthetic_batch(cfg, B, int(z["T"]), int(z[f"fwd{B}.seed_x"]), True)
    with torch.no_grad():
        out_cls, lpt, feats, w = R.forward(P, ids, mask, pixels, cfg)
    # the fixture exercises the tanh / softmax path and both sides of the ReLU (the generator's two conditions)
    assert (w[:, 0] - 0.5).abs().max().item() >= 0.25 and 0.25 <= (feats > 0).float().mean().item() <= 0.75
    assert rel(feats, t(f"fwd{B}.mm_features")) < TOL
    assert rel(out_cls, t(f"fwd{B}.out_cls")) < TOL
    assert rel(lpt, t(f"fwd{B}.logits_per_text")) < TOL


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("sfx", ["", "3"])          # the B = 4 batch, the B = 3 batch (a mixed post: text row beside image row)
@pytest.mark.parametrize("mix", ["plain", "itc"])
def test_loss_gradients_and_grad_none_set(tag, mix, sfx):
    z, cfg, P, t = load(tag)
    tr, itc, mix = "train" + sfx, mix == "itc", mix + sfx
    B, T = int(z[tr + ".B"]), int(z["T"])
    assert B == (3 if sfx else 4)
    ids, mask, onehot = t(tr + ".ids"), t(tr + ".mask"), t(tr + ".onehot")
    _, _, pixels, _ = O.synthetic_batch(cfg, B, T, int(z[tr + ".seed_x"]), True)
    keep = {}
    out_cls, loss, feats, G = R.loss_and_grads(P, ids, mask, pixels, onehot, t(tr + ".class_weight"), cfg, itc, float(z[tr + ".beta_itc"]), keep=keep)
    # d b is a sum of terms of both signs: the generator keeps it at a quarter of their magnitude sum at least, so the one-element tensor is
    # reproducible to the same relative bound as every other
    assert G[R.ASPECT_B].abs().item() >= 0.25 * keep["pre"].grad.abs().sum().item()
    assert rel(out_cls, t(f"{mix}.out_cls")) < TOL and rel(feats, t(f"{mix}.mm_features")) < TOL
    assert abs(loss.item() - float(z[f"{mix}.loss"])) / float(z[f"{mix}.loss"]) < TOL
    # grad None: the same set (the reference lists its requires_grad parameters: the frozen image tower is not among them)
    none_ref = set(str(k) for k in z[f"{mix}.grad_none"])
    none_own = {k for k, g in G.items() if g is None and "vision_model" not in k}
    assert none_own == none_ref
    assert {"linear_fusion.weight", "fc_Q.weight", "fc_K.bias", "fc_V.weight", "linear_gmu_t.weight", "linear_iadds.bias", "linear_tim.weight"} <= none_ref
    assert not any(k.startswith(("aspectattention.", "dual_encoder.text_model.pooler.")) for k in none_ref)
    assert ("dual_encoder.logit_scale" in none_ref) == (not itc)
    for k in (str(x) for x in z["watch"]):
        if k in none_ref:
            assert f"{mix}.gnorm.{k}" not in z.files
            continue
        g = G[k]
        assert abs(g.norm().item() - float(z[f"{mix}.gnorm.{k}"])) <= TOL * float(z[f"{mix}.gnorm.{k}"]), k
        if k.endswith("word_embeddings.weight"):
            sl = g[t(f"{mix}.gslice_rows.{k}")][:, :48]
            assert g[cfg.pad_id].norm().item() == pytest.approx(float(z[f"{mix}.gpad_row_norm"]), abs=1e-12)
        else:
            sl = g[:8, :48] if g.dim() == 2 else g.flatten()[:64]
        # per-tensor: a slice is held to TOL of the whole tensor's largest element
        assert (sl - t(f"{mix}.gslice.{k}")).abs().max().item() <= TOL * g.abs().max().item(), k
    assert float(z[f"{mix}.gnorm.aspectattention.weight"]) > 0 and float(z[f"{mix}.gnorm.dual_encoder.text_model.pooler.dense.weight"]) > 0


@pytest.mark.parametrize("B,H", [(1, 128), (2, 128), (3, 768), (8, 768)])
def test_operator_reference_backward_is_autograd_in_float64(B, H):
    g = torch.Generator().manual_seed(100 * B + H)
    t_pool, v_pool = (torch.tanh(torch.randn(B, H, generator=g, dtype=torch.float64)) for _ in range(2))
    a = torch.randn(H, generator=g, dtype=torch.float64) * (2.0 / H ** 0.5)
    b = torch.randn(1, generator=g, dtype=torch.float64) * 0.1
    d_feats = torch.randn(B, H, generator=g, dtype=torch.float64)
    d_t0 = torch.randn(B, H, generator=g, dtype=torch.float64)
    tp, vp, aa, bb = (x.clone().requires_grad_(True) for x in (t_pool, v_pool, a, b))
    feats, w, e = R.fusion(tp, vp, aa, bb)
    (feats * d_feats).sum().backward()
    r = R.op_reference(t_pool.numpy(), v_pool.numpy(), a.numpy(), b.numpy(), d_feats.numpy(), d_t0.numpy())
    near = lambda x, y: np.abs(np.asarray(x) - y.detach().numpy()).max() <= 1e-12 * max(1.0, np.abs(y.detach().numpy()).max())
    assert near(r["feats"], feats) and near(r["w"], w) and near(r["e"], e)
    assert near(r["d_tpool"], tp.grad + d_t0) and near(r["da"], aa.grad) and near(r["db"], bb.grad.reshape(()))
    assert np.abs(r["pre"]).max() > 1.0 and np.abs(r["w"][:, 0] - 0.5).max() > 0.1          # the softmax is not flat here
    # the reshape mixes posts: slot j of post n is row 2 n + j of [t_pool; v_pool]
    V = torch.cat((t_pool, v_pool), dim=0)
    for n in range(B):
        for j in range(2):
            assert np.array_equal(r["V"][n, j], V[2 * n + j].numpy())
    if B % 2:
        assert np.array_equal(r["V"][(B - 1) // 2, 0], t_pool[B - 1].numpy()) and np.array_equal(r["V"][(B - 1) // 2, 1], v_pool[0].numpy())
    # the bounds are finite, positive and small against the values they bound
    bd = R.op_bounds(r, a.numpy(), d_feats.numpy(), d_t0.numpy())
    for k in ("e", "w", "feats", "d_tpool", "da"):
        assert np.isfinite(bd[k]).all() and (bd[k] >= 0).all() and bd[k].max() < 1e-3 * max(1.0, np.abs(r[k]).max()), k


def test_a_wrong_row_pairing_leaves_the_bounds():
    """sensitivity of the operator bounds: the transposed reading (slot j of post n = row n of tensor j), the plausible mistake, is far outside them at
    B > 1 -- on the inputs tests/test_gpu_ops_aspect.py gives the kernel at (3, 768)"""
    B, H = 3, 768
    g = torch.Generator().manual_seed(1000 * B + H)
    t_pool, v_pool = (torch.tanh(torch.randn(B, H, generator=g)) for _ in range(2))
    a = torch.randn(H, generator=g) * (2.0 / (0.63 * H ** 0.5))
    b = torch.randn(1, generator=g) * 0.1
    r = R.op_reference(t_pool.numpy(), v_pool.numpy(), a.numpy(), b.numpy())
    bd = R.op_bounds(r, a.numpy())
    V = torch.stack((t_pool, v_pool), dim=1).double()
    e = torch.tanh(V @ a.double() + b.double())
    wrong = torch.relu((torch.softmax(e, dim=1).unsqueeze(-1) * V).sum(dim=1)).numpy()
    assert (np.abs(wrong - r["feats"]) > bd["feats"]).mean() > 0.4
