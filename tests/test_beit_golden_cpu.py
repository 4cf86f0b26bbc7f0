"""tests/beit_ref.py (the fp32 restatement of the late-fusion model with the BEiT image tower) against fixtures made by the reference's own MM_Model
over a tiny HF BeitModel (tests/golden/make_beit_golden.py): eval-mode forward at B = 1, 3, 4 for the three fusions (attention with its ITM pass),
the tower's own outputs, loss and gradients of the deterministic training cases (drop path 0) and the grad-None set -- within 2e-5, the bound
test_aspect_golden_cpu.py holds its restatement to (measured worst: 7.1e-7 on outputs, 4.5e-6 on gradient slices) -- and the relative position index
against HF's for 2 x 2, 4 x 4 and 14 x 14 windows.  The drop-path draws of the restatement: a pure function of (seed, layer, branch, post) with the
keep rate the hash owes."""
import ast
import os

import numpy as np
import pytest
import torch

from oracle import mm_oracle as O
import beit_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 2e-5
TAGS = ["beit_small_xlmr", "beit_small_bert"]
FUSIONS = ["attention", "concat", "aspect-att"]
MIXES = [("attention", "plain"), ("attention", "itc"), ("attention", "itm"), ("attention", "itcitm"), ("concat", "plain"), ("concat", "itc"),
         ("aspect-att", "plain"), ("aspect-att", "itc")]


def load(tag, fusion):
    z = np.load(os.path.join(GOLD, tag + ".npz"), allow_pickle=False)
    cfg = O.OracleConfig(**ast.literal_eval(str(z[f"{fusion}.cfg"])))
    return z, cfg, R.make_params(cfg, int(z["seed_w"])), (lambda k: torch.from_numpy(z[k]))


def rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


@pytest.mark.parametrize("W", [2, 4, 14])
def test_relative_position_index_is_hfs(W):
    z = np.load(os.path.join(GOLD, "beit_small_xlmr.npz"), allow_pickle=False)
    own = R.relative_position_index(W, W)
    assert own.shape == (W * W + 1, W * W + 1) and np.array_equal(own, z[f"hf_index.{W}"].astype(np.int64))
    n = (2 * W - 1) ** 2 + 3
    assert own.max() == n - 1 and own.min() == 0 and (own[0, 1:] == n - 3).all() and (own[1:, 0] == n - 2).all()
    assert not np.array_equal(own, own.T)          # asymmetric in (query, key): a transposed bias is another bias
    # the shipped front end computes the same buffer (vectorised)
    from smtc_amd.mm_late import beit_relative_position_index
    assert np.array_equal(beit_relative_position_index(W, W).numpy(), own)


def test_fixture_is_the_configuration_the_tower_is_built_for():
    z, cfg, P, t = load("beit_small_xlmr", "attention")
    assert (cfg.hidden, cfg.heads, cfg.layers_img, cfg.image, cfg.patch, cfg.img_kind) == (128, 2, 2, 64, 16, "beit")
    assert float(z["stochastic.diff"]) > 1e-4          # the reference's frozen tower is stochastic under model.train()
    tab = P[R.VM + "encoder.layer.0." + R.TABLE]
    assert tab.shape == (52, 2) and tab.abs().mean().item() > 0.2          # bias of the order of the scores: a missing bias cannot hide
    lam = P[R.VM + "encoder.layer.1.lambda_2"]
    assert lam.std().item() > 0.02 and not any(k.endswith("key.bias") and "vision" in k for k in P)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("fusion", FUSIONS)
@pytest.mark.parametrize("B", [1, 3, 4])
def test_forward_restatement_matches_the_reference(tag, fusion, B):
    z, cfg, P, t = load(tag, fusion)
    k = f"{fusion}.fwd{B}."
    ids, mask = t(k + "ids"), t(k + "mask")
    pixels = O.synthetic_batch(cfg, B, int(z["T"]), int(z[k + "seed_x"]), True)[2]
    tim = (t(k + "tim_ids"), t(k + "tim_mask")) if fusion == "attention" else None
    with torch.no_grad():
        x_v, v_pool = R.beit_forward(P, pixels, cfg)
        out_cls, lpt, out_tim, _, feats = R.mm_forward(P, ids, mask, pixels, cfg, tim)
    errs = dict(last_hidden=rel(x_v[0], t(k + "vit_last_hidden_post0")), pooler=rel(v_pool[0], t(k + "vit_pooler_post0")),
                out_cls=rel(out_cls, t(k + "out_cls")), lpt=rel(lpt, t(k + "logits_per_text")), feats=rel(feats, t(k + "mm_features")))
    if tim is not None:
        errs["out_tim"] = rel(out_tim, t(k + "out_tim"))
    print("BEIT_REF_FWD", tag, fusion, B, {a: float("%.3g" % b) for a, b in errs.items()})
    assert max(errs.values()) < TOL, errs
    assert 0.25 <= (feats > 0).float().mean().item() <= 0.75


def test_the_bias_and_the_layer_scale_are_visible_in_the_fixture():
    """sensitivity: the restatement without the bias, with the bias transposed, or with lambda = 0.1 everywhere is far outside the tolerance"""
    z, cfg, P, t = load("beit_small_xlmr", "attention")
    k = "attention.fwd3."
    pixels = O.synthetic_batch(cfg, 3, int(z["T"]), int(z[k + "seed_x"]), True)[2]
    ref = t(k + "vit_last_hidden_post0")
    idx = torch.from_numpy(R.relative_position_index(4, 4))
    for what in ("nobias", "transposed", "lambda"):
        Q = dict(P)
        for l in range(cfg.layers_img):
            p = f"{R.VM}encoder.layer.{l}."
            if what == "nobias":
                Q[p + R.TABLE] = torch.zeros_like(P[p + R.TABLE])
            if what == "lambda":
                Q[p + "lambda_1"] = torch.full_like(P[p + "lambda_1"], 0.1)
        with torch.no_grad():
            if what == "transposed":
                orig = R.relative_position_index
                R.relative_position_index = lambda a, b: orig(a, b).T.copy()
                try:
                    x = R.beit_forward(Q, pixels, cfg)[0]
                finally:
                    R.relative_position_index = orig
            else:
                x = R.beit_forward(Q, pixels, cfg)[0]
        assert rel(x[0], ref) > 100 * TOL, what
    assert idx.shape == (17, 17)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("fusion,mix", MIXES)
def test_loss_gradients_and_grad_none_set(tag, fusion, mix):
    z, cfg, P, t = load(tag, fusion)
    cfg0 = O.OracleConfig(**{**O.asdict(cfg), "p_hidden": 0.0, "p_attn": 0.0, "p_head": 0.0})
    tr, m = f"{fusion}.train.", f"{fusion}.{mix}."
    itc, itm = mix in ("itc", "itcitm"), mix in ("itm", "itcitm")
    B, T = int(z[tr + "B"]), int(z["T"])
    pixels = O.synthetic_batch(cfg0, B, T, int(z[tr + "seed_x"]), True)[2]
    tim = (t(tr + "tim_ids"), t(tr + "tim_mask"), t(tr + "lbl_tim"))
    out_cls, loss, feats, out_tim, G = R.loss_and_grads(P, t(tr + "ids"), t(tr + "mask"), pixels, t(tr + "onehot"), t(tr + "class_weight"), cfg0, itc, itm, tim,
                                                        float(z[tr + "beta_itc"]), float(z[tr + "beta_itm"]))
    assert rel(out_cls, t(m + "out_cls")) < TOL and rel(feats, t(m + "mm_features")) < TOL
    if itm:
        assert rel(out_tim, t(m + "out_tim")) < TOL
    assert abs(loss.item() - float(z[m + "loss"])) / float(z[m + "loss"]) < TOL
    none_ref = set(str(k) for k in z[m + "grad_none"])
    none_own = {k for k, g in G.items() if g is None and "vision_model" not in k}
    assert none_own == none_ref
    assert all(G[k] is None for k in G if "vision_model" in k)          # the tower is frozen
    worst = 0.0
    for k in (str(x) for x in z["watch"]):
        if k in none_ref:
            assert m + f"gnorm.{k}" not in z.files
            continue
        g = G[k]
        gn = float(z[m + f"gnorm.{k}"])
        assert abs(g.norm().item() - gn) <= TOL * gn, k
        sl = g[t(m + f"gslice_rows.{k}")][:, :48] if k.endswith("word_embeddings.weight") else (g[:8, :48] if g.dim() == 2 else g.flatten()[:64])
        e = (sl - t(m + f"gslice.{k}")).abs().max().item() / g.abs().max().item()
        worst = max(worst, e)
        assert e <= TOL, (k, e)
    print("BEIT_REF_GRAD", tag, fusion, mix, "worst %.3g" % worst)


# ---------------------------------------------------------------------------------------------------- stochastic depth: the draws
def test_drop_path_draws_are_a_pure_function_with_the_right_rate():
    seed, posts = 0x9E3779B97F4A7C15 + 7, 4096
    for layers, rate in ((12, 0.1), (2, 0.5)):
        for l in range(layers):
            p = float(R.drop_path_p(rate, l, layers))
            assert abs(p - rate * l / (layers - 1)) < 1e-7
            for branch in (0, 1):
                keep, scale = R.droppath_keep(seed, l, branch, posts, p)
                again, _ = R.droppath_keep(seed, l, branch, posts, p)
                assert np.array_equal(keep, again)                       # a function of its arguments alone
                assert np.array_equal(keep[:100], R.droppath_keep(seed, l, branch, 100, p)[0])          # ... and of the post, not of the batch size
                if p == 0:
                    assert keep.all() and scale == 1.0
                    continue
                q = 1.0 - R.drop_threshold16(p) / 65536.0
                assert abs(q - (1 - p)) < 1e-5 and abs(scale * q - 1.0) < 1e-6
                sd = (posts * q * (1 - q)) ** 0.5
                assert abs(int(keep.sum()) - posts * q) <= 4 * sd, (l, branch, int(keep.sum()), posts * q, sd)
    # the two branches of a layer, and two layers, draw independently: their keep patterns differ
    a = R.droppath_keep(seed, 1, 0, posts, 0.5)[0]
    assert not np.array_equal(a, R.droppath_keep(seed, 1, 1, posts, 0.5)[0]) and not np.array_equal(a, R.droppath_keep(seed, 2, 0, posts, 0.5)[0])
    assert not np.array_equal(a, R.droppath_keep(seed + 1, 1, 0, posts, 0.5)[0])
    assert abs(np.mean(a == R.droppath_keep(seed, 1, 1, posts, 0.5)[0]) - 0.5) < 4 * 0.5 / posts ** 0.5


def test_drop_path_replay_in_the_restatement():
    """rate 0.5 on the 2-layer model: layer 0 never drops; a post with both branches of layer 1 dropped leaves the tower with its layer-0 output, a
    kept branch enters scaled by 2"""
    z, cfg, P, t = load("beit_small_xlmr", "attention")
    B, seed = 16, 1234567
    pixels = O.synthetic_batch(cfg, B, int(z["T"]), 99, True)[2]
    with torch.no_grad():
        layers = []
        x_eval = R.beit_forward(P, pixels, cfg, None, layers)[0]
        x_tr = R.beit_forward(P, pixels, cfg, (0.5, seed))[0]
    k0, s0 = R.droppath_keep(seed, 1, 0, B, 0.5)
    k1, s1 = R.droppath_keep(seed, 1, 1, B, 0.5)
    assert s0 == 2.0 and s1 == 2.0
    both = ~k0 & ~k1
    assert both.any() and (k0 & k1).any()
    for b in range(B):
        if both[b]:
            assert torch.equal(x_tr[b], layers[0][b])
        elif k0[b] or k1[b]:
            assert not torch.allclose(x_tr[b], x_eval[b])
