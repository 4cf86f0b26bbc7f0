"""tests/img_ref.py (the fp32 restatement of the reference's image-only model) against the fixture made with the reference's own code path
(tests/golden/make_img_golden.py): logits, loss, gradients, one AdamW step -- within 2e-5, test_txt_golden_cpu.py's method and bound."""
import ast
import os

import numpy as np
import torch

from oracle import mm_oracle as O
import img_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 2e-5


def rel_l2(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def test_restatement_matches_the_reference():
    path = os.path.join(GOLD, "img_small_vit.npz")
    assert os.path.getsize(path) < 800 * 1024
    z = np.load(path, allow_pickle=False)
    cfg = O.OracleConfig(**ast.literal_eval(str(z["cfg"])))
    t = lambda k: torch.from_numpy(z[k])
    P = R.make_params(cfg, 0)
    assert cfg.image == 192 and cfg.img_tokens == 145 and int(z["B"]) == 2 and cfg.layers_img == 2
    assert [str(k) for k in z["keys"]] == sorted(P)
    assert z["pixels_u8"].dtype == np.uint8
    px = R.from_u8(t("pixels_u8"))
    with torch.no_grad():
        logits = R.forward(P, px, cfg)
    assert rel_l2(logits, t("logits")) < TOL
    r_logits, loss, G = R.loss_and_grads(P, px, t("onehot"), t("class_weight"), cfg)
    assert rel_l2(r_logits, t("train_logits")) < TOL
    assert abs(loss.item() - float(z["loss"])) / float(z["loss"]) < TOL
    M = {k: torch.zeros_like(v) for k, v in P.items()}
    V = {k: torch.zeros_like(v) for k, v in P.items()}
    after = {k: v.clone() for k, v in P.items()}
    lr, eps = float(z["lr"]), 1e-8
    R.adamw(after, G, M, V, 1, lr, float(z["weight_decay"]))
    worst, share = 0.0, 0.0
    for k in (str(x) for x in z["watch"]):
        g, gg = R.pick(k, G[k]), t("grad." + k)
        assert g.shape == gg.shape, k
        if k.endswith("attention.attention.key.bias"):
            # softmax is invariant to a shift of the scores along the keys, which is all a key bias does: its gradient is zero in exact arithmetic and
            # both sides hold rounding residue -- bounded against the same layer's query-bias gradient; Adam turns residue into +-lr: not compared
            q = R.pick(k, G[k.replace(".key.", ".query.")]).abs().max()
            assert g.abs().max() < 1e-5 * q and gg.abs().max() < 1e-5 * t("grad." + k.replace(".key.", ".query.")).abs().max(), k
            continue
        e = rel_l2(g, gg)
        worst = max(worst, e)
        assert e < TOL, (k, e)
        # Adam's first step moves an element by lr g / (|g| + eps): Lipschitz in g with constant lr eps / ((|g| + eps)(|g'| + eps))
        a, aa = R.pick(k, after[k]), t("after." + k)
        slack = lr * eps * (g - gg).abs() / ((g.abs() + eps) * (gg.abs() + eps))
        bound = TOL * aa.abs().max() + slack
        assert ((a - aa).abs() <= bound).all(), k
        s = (slack > TOL * aa.abs().max()).float().mean().item()
        share = max(share, s)
        assert s < 0.05, k                                           # the amplified elements are few
        assert (aa - R.pick(k, P[k])).abs().max().item() > 0.5 * lr          # the step moved the watched rows
    print(f"worst gradient rel L2 {worst:.2e}, largest share of slack-needing elements {share:.4f}")
