#!/usr/bin/env python3
"""Golden vectors of the late-fusion model under --fusion_name aspect-att, made by running the REFERENCE's own MM_Model (models/mm_late.py:115-131;
needs the reference checkout next to this tree, CPU only).  The shim, the random-init directory recipe and the weight loader are make_golden.py's,
imported unchanged.

Writes tests/golden/aspect_small_xlmr.npz and aspect_small_bert.npz (2 + 2 layers, T = 32, padded rows; images are regenerated from the seed):
  fwd<B>.*    eval-mode forward at B = 1, 3, 4: ids, mask, out_cls, logits_per_text, mm_features
  plain.* / itc.*   train mode, every dropout p = 0 (as make_golden.py's training cases), B = 4 (inputs under train.*), class weights; without
              ITC and with it (beta_itc = 0.1): loss, out_cls, gnorm.<name> / gslice.<name> of the watched parameters in train_small_xlmr.npz's
              layout, grad_none
  plain3.* / itc3.* the same at B = 3 (inputs under train3.*): B = 4 pairs text with text and image with image only; here post 1 holds
              (t_pool[2], v_pool[0]), the mixed post and the odd tail, so d t_pool of a text row beside an image row -- with ITC's share added --
              is in the gradients

With oracle.make_params as it stands the two softmax weights stay within 0.05 of 1/2 and the tanh / softmax path is hardly visible in the outputs.
aspectattention.weight is therefore multiplied by `aspect_scale`, the smallest power of two at which some post of EVERY stored case has
|w_0 - 1/2| >= 0.25 (|e_0 - e_1| >= ln 3; e = tanh(.) lies in (-1, 1), so a post gets there only if its two pre-tanh values differ in sign or one of
them is near zero: an input seed whose batch has no such post is replaced by seed + 100, + 200, ... -- B = 4 pairs text with text and image with
image only); the share of positive mm_features units must then still lie in [0.25, 0.75].  A third condition holds for the training batches:
d aspectattention.bias = sum_n (dpre_n0 + dpre_n1) is a sum of terms of both signs (dpre_n0 = -ds (1 - e_0^2), dpre_n1 = +ds (1 - e_1^2)), and a
batch on which they nearly cancel leaves a one-element tensor that no fp32 evaluation reproduces to a relative 2e-5; |d b| is at least a quarter
of sum |dpre| (a seed that misses it is replaced as above).  The other one-element tensor, d logit_scale = sum_ij G_ij L_ij (G = d loss / d logits,
whose rows and columns sum to zero, against logits that are nearly equal at random initialisation), cancels by construction: shares of 0.002 to
0.17 over seeds.  Two fp32 evaluations agree on its terms to about 5e-7 (a few roundings of a 512-long normalised dot and a softmax), so the sum
is reproducible to 2e-5 from a share of 0.025 on; batches under 0.03 are replaced.  All conditions are asserted here.
Nothing of the reference is copied: the files are data.   Run:  python tests/golden/make_aspect_golden.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))
from make_golden import install_shim, build_reference_model, load_params, grads_by_ref_key, O  # noqa: E402
import aspect_ref as R  # noqa: E402

T = 32
FWD = {1: 41, 3: 42, 4: 43}          # B -> first input seed tried
TRAIN = {"": (4, 44), "3": (3, 45)}          # key suffix -> (B, first input seed tried)
DB_SHARE, LS_SHARE = 0.25, 0.03
CLASS_W = [0.7, 1.6, 0.9, 1.1]
# The scale also multiplies whatever rounding the pooler outputs carry on their way into the tanh, and 1 - e^2 = sech^2 is the more sensitive to it
# the further it saturates (relative change 2 tanh(x) dx): a fixture at scale 32 measures that conditioning (the fp32 parity mode itself then sits
# ten times further from the reference on aspectattention.* than on any other tensor), not the kernels.  The scale is therefore capped at 8 and the
# input seeds are searched instead.
SCALES = [1.0, 2.0, 4.0, 8.0]
WATCH = ["linear_cls.weight", "linear_cls.bias", "aspectattention.weight", "aspectattention.bias", "linear_fusion.bias", "fc_Q.weight",
         "linear_tim.weight", "dual_encoder.logit_scale", "dual_encoder.text_projection.weight", "dual_encoder.visual_projection.weight",
         "dual_encoder.text_model.pooler.dense.weight", "dual_encoder.text_model.pooler.dense.bias",
         "dual_encoder.text_model.encoder.layer.0.attention.self.query.weight",
         "dual_encoder.text_model.encoder.layer.0.attention.self.value.weight",
         "dual_encoder.text_model.encoder.layer.0.attention.output.LayerNorm.weight",
         "dual_encoder.text_model.encoder.layer.0.intermediate.dense.bias",
         "dual_encoder.text_model.encoder.layer.1.output.dense.weight",
         "dual_encoder.text_model.encoder.layer.1.output.LayerNorm.bias",
         "dual_encoder.text_model.embeddings.LayerNorm.weight",
         "dual_encoder.text_model.embeddings.position_embeddings.weight",
         "dual_encoder.text_model.embeddings.word_embeddings.weight"]


def params(cfg, seed_w, scale):
    P = O.make_params(cfg, seed_w)
    P[R.ASPECT_W] = P[R.ASPECT_W] * scale
    return P


def spread(P, cfg, B, seed_x):
    ids, mask, pixels, _ = O.synthetic_batch(cfg, B, T, seed_x, True)
    with torch.no_grad():
        _, _, feats, w = R.forward(P, ids, mask, pixels, cfg)
    return (w[:, 0] - 0.5).abs().max().item(), (feats > 0).float().mean().item()


def pre_tanh_dots(P, cfg, B, seed_x):
    """V a of the batch at scale 1 (it is linear in the scale)"""
    ids, mask, pixels, _ = O.synthetic_batch(cfg, B, T, seed_x, True)
    with torch.no_grad():
        _, v = O.vit_forward(P, pixels, cfg, None)
        _, t = O.text_forward(P, ids, mask, cfg, O.Dropout("none"), 0, None)
    return (torch.cat((t, v), dim=0) @ P[R.ASPECT_W].reshape(-1)).reshape(B, 2)


def spread_at(d, b, scale):
    return (torch.softmax(torch.tanh(d * scale + b), dim=1)[:, 0] - 0.5).abs().max().item()


def db_share(cfg0, seed_w, scale, B, seed_x, itc):
    """|d b| / sum |dpre| of a training batch (the restatement; dropout off)"""
    ids, mask, pixels, onehot = O.synthetic_batch(cfg0, B, T, seed_x, True)
    keep = {}
    _, _, _, G = R.loss_and_grads(params(cfg0, seed_w, scale), ids, mask, pixels, onehot, torch.tensor(CLASS_W[: cfg0.num_labels]), cfg0, itc, 0.1, keep=keep)
    return G[R.ASPECT_B].abs().item() / keep["pre"].grad.abs().sum().item()


def ls_share(cfg0, seed_w, scale, B, seed_x):
    """|d logit_scale| / sum |G_ij L_ij| of a training batch with ITC (the restatement; logits = cos * exp(logit_scale), so d logits / d logit_scale
    = logits)"""
    ids, mask, pixels, onehot = O.synthetic_batch(cfg0, B, T, seed_x, True)
    Pg = {k: v.clone().requires_grad_(R.trainable(k, True)) for k, v in params(cfg0, seed_w, scale).items()}
    out_cls, lpt, _, _ = R.forward(Pg, ids, mask, pixels, cfg0)
    lpt.retain_grad()
    O.mix_loss(out_cls, onehot, torch.tensor(CLASS_W[: cfg0.num_labels]), lpt, None, None, True, False, 0.1).backward()
    terms = (lpt.grad * lpt).detach()
    return terms.sum().abs().item() / terms.abs().sum().item()


def choose(cfg, cfg0, seed_w):
    """-> ({B: seed}, {suffix: train seed}, scale): per case the first seed with a post that reaches the spread at the largest scale, then the smallest
    common scale; a training batch whose d b misses its share at that scale moves on to the next seed that has both at that scale"""
    P = O.make_params(cfg, seed_w)
    b = P[R.ASPECT_B].reshape(())
    cases = {**{B: (B, s) for B, s in FWD.items()}, **{"train" + sfx: v for sfx, v in TRAIN.items()}}
    picked = {}
    for key, (B, seed) in cases.items():
        while spread_at(pre_tanh_dots(P, cfg, B, seed), b, SCALES[-1]) < 0.25:
            seed += 100
            assert seed < 6000, "softmax spread not reachable"
        picked[key] = seed
    scale = next(s for s in SCALES if all(spread_at(pre_tanh_dots(P, cfg, cases[k][0], seed), b, s) >= 0.25 for k, seed in picked.items()))
    for sfx, (B, _) in TRAIN.items():
        seed = picked["train" + sfx]
        while spread_at(pre_tanh_dots(P, cfg, B, seed), b, scale) < 0.25 or min(db_share(cfg0, seed_w, scale, B, seed, itc) for itc in (False, True)) < DB_SHARE or \
                ls_share(cfg0, seed_w, scale, B, seed) < LS_SHARE:
            seed += 100
            assert seed < 6000, "shares of d b / d logit_scale not reachable"
        picked["train" + sfx] = seed
    return {B: picked[B] for B in FWD}, {sfx: picked["train" + sfx] for sfx in TRAIN}, scale


def case(tag, cfg, txt_name, seed_w, ref_config):
    import utils as ref_utils
    cfg0 = O.OracleConfig(**{**O.asdict(cfg), "p_hidden": 0.0, "p_attn": 0.0, "p_head": 0.0})
    fwd_seeds, train_seeds, scale = choose(cfg, cfg0, seed_w)
    P = params(cfg, seed_w, scale)
    out = dict(cfg=np.array(repr(O.asdict(cfg))), T=T, seed_w=seed_w, aspect_scale=scale, watch=np.array(WATCH))
    with tempfile.TemporaryDirectory() as tmp:
        _, model = build_reference_model(ref_config, cfg, txt_name, tmp, 0.1)
    load_params(model, P)
    model.eval()
    for B, seed_x in fwd_seeds.items():
        ids, mask, pixels, onehot = O.synthetic_batch(cfg, B, T, seed_x, True)
        with torch.no_grad():
            out_cls, lpt, out_tim, _, feats = model(ids, mask, pixels)
        assert out_tim is None
        sp, pos = spread(P, cfg, B, seed_x)
        assert sp >= 0.25, (tag, B, sp)
        assert 0.25 <= pos <= 0.75 and 0.25 <= (feats > 0).float().mean().item() <= 0.75, (tag, B, pos)
        out.update({f"fwd{B}.seed_x": seed_x, f"fwd{B}.ids": ids.numpy(), f"fwd{B}.mask": mask.numpy(), f"fwd{B}.onehot": onehot.numpy(),
                    f"fwd{B}.out_cls": out_cls.numpy(), f"fwd{B}.logits_per_text": lpt.numpy(), f"fwd{B}.mm_features": feats.numpy(),
                    f"fwd{B}.spread": sp, f"fwd{B}.positive": pos})
        print(tag, "fwd", B, "spread", round(sp, 3), "positive", round(pos, 3), "out_cls", out_cls.flatten()[:3].tolist())
    # ---- training cases: dropout off, the reference's own losses
    with tempfile.TemporaryDirectory() as tmp:
        _, model = build_reference_model(ref_config, cfg0, txt_name, tmp, 0.0)
    load_params(model, P)
    model.train()
    w = torch.tensor(CLASS_W[: cfg0.num_labels])
    loss_fn = torch.nn.CrossEntropyLoss(weight=w)            # run_mm_late.py:85
    for sfx, (TRAIN_B, _) in TRAIN.items():
        train_seed = train_seeds[sfx]
        ids, mask, pixels, onehot = O.synthetic_batch(cfg0, TRAIN_B, T, train_seed, True)
        sp, pos = spread(P, cfg0, TRAIN_B, train_seed)
        assert sp >= 0.25 and 0.25 <= pos <= 0.75, (tag, sp, pos)
        shares = [db_share(cfg0, seed_w, scale, TRAIN_B, train_seed, itc) for itc in (False, True)]
        assert min(shares) >= DB_SHARE and ls_share(cfg0, seed_w, scale, TRAIN_B, train_seed) >= LS_SHARE, (tag, sfx, shares)
        out.update({f"train{sfx}.B": TRAIN_B, f"train{sfx}.seed_x": train_seed, f"train{sfx}.ids": ids.numpy(), f"train{sfx}.mask": mask.numpy(), f"train{sfx}.onehot": onehot.numpy(),
                    f"train{sfx}.class_weight": w.numpy(), f"train{sfx}.spread": sp, f"train{sfx}.positive": pos, f"train{sfx}.beta_itc": 0.1})
        for mix, itc in (("plain", False), ("itc", True)):
            model.zero_grad(set_to_none=True)
            o, lpt, _, _, feats = model(ids, mask, pixels)
            label = onehot.type_as(o)                            # mm_late.py:471
            loss = (1 - 0.1) * loss_fn(o, label) + 0.1 * ref_utils.clip_loss(lpt) if itc else loss_fn(o, label)      # mm_late.py:473-487
            loss.backward()
            out[f"{mix}{sfx}.loss"] = loss.item()
            out[f"{mix}{sfx}.out_cls"] = o.detach().numpy()
            out[f"{mix}{sfx}.mm_features"] = feats.detach().numpy()
            G = grads_by_ref_key(model, WATCH)
            out[f"{mix}{sfx}.grad_none"] = np.array(sorted(n for n, q in model.named_parameters() if q.requires_grad and q.grad is None))
            for k in WATCH:
                g = G.get(k)
                if g is None:
                    continue
                out[f"{mix}{sfx}.gnorm.{k}"] = g.norm().item()
                if k.endswith("word_embeddings.weight"):
                    touched = torch.unique(ids)[:6]
                    out[f"{mix}{sfx}.gslice.{k}"] = g[touched][:, :48].numpy()
                    out[f"{mix}{sfx}.gslice_rows.{k}"] = touched.numpy()
                    out[f"{mix}{sfx}.gpad_row_norm"] = g[cfg0.pad_id].norm().item()
                elif g.dim() == 2:
                    out[f"{mix}{sfx}.gslice.{k}"] = g[:8, :48].numpy()
                else:
                    out[f"{mix}{sfx}.gslice.{k}"] = g.flatten()[:64].numpy()
            print(tag, mix + sfx, "loss", loss.item(), "grad None:", len(out[f"{mix}{sfx}.grad_none"]))
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= 784 * 1024
    print(tag, "aspect_scale", scale, os.path.getsize(path), "bytes")


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    rc = install_shim()
    case("aspect_small_xlmr", O.OracleConfig(layers_txt=2, layers_img=2, vocab=1000, max_pos=130, num_labels=3, fusion="aspect-att"), "bernice", 0, rc)
    case("aspect_small_bert", O.OracleConfig(layers_txt=2, layers_img=2, vocab=1000, max_pos=512, type_vocab=2, txt_kind="bert", pad_id=0,
                                             ln_eps_txt=1e-12, num_labels=2, fusion="aspect-att"), "bert", 1, rc)


if __name__ == "__main__":
    main()
