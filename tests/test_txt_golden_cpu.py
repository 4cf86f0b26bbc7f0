"""tests/txt_ref.py (the fp32 restatement of the reference's text-only modules) against fixtures made by the reference's own code
(tests/golden/make_txt_golden.py): logits, loss, gradients, one AdamW step -- within 2e-5, the bound test_oracle_golden.py holds the oracle to."""
import ast
import os

import numpy as np
import pytest
import torch

from oracle import mm_oracle as O
import txt_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 2e-5


def load(tag):
    z = np.load(os.path.join(GOLD, tag + ".npz"), allow_pickle=False)
    cfg = O.OracleConfig(**ast.literal_eval(str(z["cfg"])))
    t = lambda k: torch.from_numpy(z[k])
    return z, cfg, t


def rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


@pytest.mark.parametrize("tag", ["txt_small_xlmr", "txt_small_bert"])
def test_restatement_matches_the_reference(tag):
    z, cfg, t = load(tag)
    P = R.make_params(cfg, 0)
    tt = t("token_type_ids") if "token_type_ids" in z.files else None
    if tag.endswith("bert"):
        assert tt is not None and int(tt.sum()) > 0
    assert (t("mask") == 0).any()                                   # padded rows
    assert set(str(k) for k in z["keys"]) - {"bert_model.embeddings.position_ids", "bert_model.embeddings.token_type_ids"} == set(P)
    with torch.no_grad():
        logits = R.forward(P, t("ids"), t("mask"), tt, cfg)
    assert rel(logits, t("logits")) < TOL
    r_logits, loss, G = R.loss_and_grads(P, t("ids"), t("mask"), tt, t("onehot"), t("class_weight"), cfg)
    assert rel(r_logits, t("train_logits")) < TOL
    assert abs(loss.item() - float(z["loss"])) / float(z["loss"]) < TOL
    M = {k: torch.zeros_like(v) for k, v in P.items()}
    V = {k: torch.zeros_like(v) for k, v in P.items()}
    after = {k: v.clone() for k, v in P.items()}
    R.adamw(after, G, M, V, 1, float(z["lr"]), float(z["weight_decay"]))
    for k in (str(x) for x in z["watch"]):
        rows = t("rows." + k) if "rows." + k in z.files else None
        pick = (lambda x: x) if rows is None else (lambda x: x[rows])
        if k.endswith("word_embeddings.weight"):                     # every word row that occurs is held
            assert torch.equal(rows, torch.unique(t("ids")))
        if bool(z["nograd." + k]):
            assert G[k] is None and ".pooler." in k                  # computed by the reference, never consumed
            assert torch.equal(pick(after[k]), pick(P[k])) and torch.equal(t("after." + k), pick(P[k]))
            continue
        if k.endswith("attention.self.key.bias"):
            # softmax is invariant to a shift of the scores along the keys, which is all a key bias does: its gradient is zero in exact arithmetic,
            # both sides hold rounding residue (and Adam's normalised first step of a residue is +-lr noise: not compared)
            assert pick(G[k]).abs().max() < 1e-8 and t("grad." + k).abs().max() < 1e-8
            continue
        assert rel(pick(G[k]), t("grad." + k)) < TOL, k
        # Adam's first step moves an element by lr g / (|g| + eps): Lipschitz in g with constant lr eps / ((|g| + eps)(|g'| + eps)) -- where the gradient
        # is within a few eps of zero, the 2e-5 the gradients agree to is amplified; the bound per element is that constant times |g - g'|
        g, gg, eps, lr = pick(G[k]), t("grad." + k), 1e-8, float(z["lr"])
        if "arows." + k in z.files:                                  # the stepped rows are the first of the gradient's rows
            arows = t("arows." + k)
            assert torch.equal(arows, rows[:arows.numel()])
            g, gg = g[:arows.numel()], gg[:arows.numel()]
            pick = lambda x: x[arows]
        slack = lr * eps * (g - gg).abs() / ((g.abs() + eps) * (gg.abs() + eps))
        bound = TOL * t("after." + k).abs().max() + slack
        assert ((pick(after[k]) - t("after." + k)).abs() <= bound).all(), k
        assert (slack > TOL * t("after." + k).abs().max()).float().mean() < 0.05, k          # the amplified elements are few
        step = (t("after." + k) - pick(P[k])).abs().max().item()
        assert step > 0.5 * float(z["lr"])                           # the step moved the watched rows (Adam's first step is ~lr per element)
