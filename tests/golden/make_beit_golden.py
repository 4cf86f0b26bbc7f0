#!/usr/bin/env python3
"""Golden vectors of the late-fusion model with --img_model_name beit, made by running the REFERENCE's own MM_Model (models/mm_late.py:50-193) over a
tiny random HF BeitModel (needs the reference checkout next to this tree and the installed transformers; CPU only).  The shim is make_golden.py's,
imported unchanged; the reference hard-wires its head widths to 768 (models/config.py:82-84), so those three module constants are set to the tiny
width before its MM_Model is built -- the same kind of shim as make_golden.py's `config.T`.

Writes tests/golden/beit_small_xlmr.npz and beit_small_bert.npz: both towers 128 wide, 2 heads, 2 layers, MLP 256; images 64 x 64 in 16 x 16 patches
(17 tokens, a 4 x 4 window); T = 32 with padded rows; images are regenerated from the seed.  The BEiT tower has the configuration of
microsoft/beit-base-patch16-224-pt22k-ft22k (no absolute positions, per-layer relative position bias, mean pooling, layer scale 0.1, drop path 0.1)
and the weights of tests/beit_ref.py make_params: lambda_*, the bias tables and the pooler LayerNorm are non-trivial (HF's own initialisation
leaves the bias at zero and a test blind to it).
  <fusion>.fwd<B>.*     eval-mode forward at B = 1, 3, 4 for attention, concat, aspect-att: ids, mask, out_cls, logits_per_text, mm_features; attention
                        also with the ITM pass (tim_ids, tim_mask, out_tim); vision last_hidden_state / pooler_output of post 0
  <fusion>.<mix>.*      train mode with drop_path_rate = 0 and every dropout p = 0 (deterministic), B = 4, class weights: plain, itc (beta 0.1) and,
                        for attention, itm and itcitm: loss, out_cls, mm_features, gnorm.<name> / gslice.<name> of the watched parameters, grad_none
  hf_index.<W>          HF's own relative position index for W x W windows (W = 2, 4, 14), which tests/beit_ref.py's is held to
  stochastic.diff       max |pooler_output difference| of two train-mode forwards of the reference's tower at drop_path_rate 0.1 (> 0: the frozen tower
                        is stochastic under model.train())
Nothing of the reference is copied: the files are data.   Run:  python tests/golden/make_beit_golden.py"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from make_golden import install_shim, O  # noqa: E402
import beit_ref as R  # noqa: E402

T = 32
FWD = {1: 51, 3: 52, 4: 53}
TRAIN_B, TRAIN_SEED = 4, 54
CLASS_W = [0.7, 1.6, 0.9, 1.1]
FUSIONS = ["attention", "concat", "aspect-att"]
WATCH = ["linear_cls.weight", "linear_cls.bias", "linear_tim.weight", "linear_fusion.weight", "linear_fusion.bias", "fc_Q.weight", "fc_K.weight", "fc_V.weight",
         "fc_V.bias", "aspectattention.weight", "aspectattention.bias", "dual_encoder.logit_scale", "dual_encoder.text_projection.weight",
         "dual_encoder.visual_projection.weight", "dual_encoder.text_model.pooler.dense.weight",
         "dual_encoder.text_model.encoder.layer.0.attention.self.query.weight",
         "dual_encoder.text_model.encoder.layer.0.attention.self.value.weight",
         "dual_encoder.text_model.encoder.layer.0.attention.output.LayerNorm.weight",
         "dual_encoder.text_model.encoder.layer.0.intermediate.dense.bias",
         "dual_encoder.text_model.encoder.layer.1.output.dense.weight",
         "dual_encoder.text_model.encoder.layer.1.output.LayerNorm.bias",
         "dual_encoder.text_model.embeddings.LayerNorm.weight",
         "dual_encoder.text_model.embeddings.position_embeddings.weight",
         "dual_encoder.text_model.embeddings.word_embeddings.weight"]


def to_hf5_key(k):
    """4.25.1 checkpoint key -> key of the installed transformers (the BEiT renames; the text tower keeps its names)"""
    from smtc_amd.mm_late import _beit_ref_to_key
    vm = "dual_encoder.vision_model."
    return vm + _beit_ref_to_key(k[len(vm):]) if k.startswith(vm) else k


def build_reference_model(ref_config, cfg, txt_name, tmp, p_txt, drop_path_rate):
    from transformers import BeitConfig, BeitModel, XLMRobertaConfig, XLMRobertaModel, BertConfig, BertModel
    vdir, tdir = os.path.join(tmp, "beit"), os.path.join(tmp, txt_name)
    BeitModel(BeitConfig(hidden_size=cfg.Hv, num_attention_heads=cfg.heads_v, num_hidden_layers=cfg.layers_img, intermediate_size=cfg.Iv,
                         image_size=cfg.image, patch_size=cfg.patch, layer_norm_eps=cfg.ln_eps_img, use_absolute_position_embeddings=False,
                         use_relative_position_bias=True, use_shared_relative_position_bias=False, use_mean_pooling=True,
                         layer_scale_init_value=0.1, drop_path_rate=drop_path_rate, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)).save_pretrained(vdir)
    common = dict(vocab_size=cfg.vocab, max_position_embeddings=cfg.max_pos, hidden_size=cfg.hidden, num_attention_heads=cfg.heads,
                  intermediate_size=cfg.inter, num_hidden_layers=cfg.layers_txt, hidden_dropout_prob=p_txt, attention_probs_dropout_prob=p_txt)
    if cfg.txt_kind == "xlmr":
        XLMRobertaModel(XLMRobertaConfig(type_vocab_size=1, layer_norm_eps=cfg.ln_eps_txt, pad_token_id=1, bos_token_id=0, eos_token_id=2, **common)).save_pretrained(tdir)
    else:
        BertModel(BertConfig(type_vocab_size=2, **common)).save_pretrained(tdir)
    ref_config.MODEL_DIR_DICT["beit"] = vdir
    ref_config.MODEL_DIR_DICT[txt_name] = tdir
    import mm_late as ref_mm_late
    ref_mm_late.MODEL_DIR_DICT = ref_config.MODEL_DIR_DICT
    ref_mm_late.txt_feat_size = ref_mm_late.img_feat_size = ref_mm_late.fixed_feat_size = cfg.hidden      # models/config.py:82-84 hard-wires 768
    return ref_mm_late.MM_Model(cfg.num_labels, txt_name, "beit", cfg.p_head, cfg.fusion)


def load_params(model, P):
    sd = model.state_dict()
    mapped = {to_hf5_key(k): v for k, v in P.items()}
    missing = [k for k in sd if k not in mapped and not k.endswith("position_ids") and not k.endswith("token_type_ids")]
    extra = [k for k in mapped if k not in sd]
    assert not missing and not extra, (missing[:5], extra[:5])
    for k, v in mapped.items():
        assert tuple(sd[k].shape) == tuple(v.shape), (k, sd[k].shape, v.shape)
    model.load_state_dict(mapped, strict=False)


def grads_by_ref_key(model, names):
    inv = {to_hf5_key(k): k for k in names}
    return {inv[n]: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters() if n in inv}


def case(tag, base, txt_name, seed_w, ref_config):
    import utils as ref_utils
    out = dict(T=T, seed_w=seed_w, watch=np.array(WATCH), fusions=np.array(FUSIONS))
    from transformers.models.beit.modeling_beit import BeitRelativePositionBias
    for W in (2, 4, 14):
        out[f"hf_index.{W}"] = BeitRelativePositionBias.generate_relative_position_index((W, W)).numpy().astype(np.int32)
    w = torch.tensor(CLASS_W[: base["num_labels"]])
    loss_fn, tim_loss_fn = torch.nn.CrossEntropyLoss(weight=w), torch.nn.CrossEntropyLoss()            # run_mm_late.py:85,97
    for fusion in FUSIONS:
        cfg = O.OracleConfig(**{**base, "fusion": fusion})
        cfg0 = O.OracleConfig(**{**O.asdict(cfg), "p_hidden": 0.0, "p_attn": 0.0, "p_head": 0.0})
        out[f"{fusion}.cfg"] = np.array(repr(O.asdict(cfg)))
        P = R.make_params(cfg, seed_w)
        with tempfile.TemporaryDirectory() as tmp:
            model = build_reference_model(ref_config, cfg, txt_name, tmp, 0.1, 0.1)
        load_params(model, P)
        model.eval()
        for B, seed_x in FWD.items():
            ids, mask, pixels, onehot = O.synthetic_batch(cfg, B, T, seed_x, True)
            np.random.seed(30 + B)
            tim_ids, tim_mask, lbl_tim = O.prepare_itm_inputs(ids, mask)
            itm = fusion == "attention"
            with torch.no_grad():
                out_cls, lpt, out_tim, _, feats = model(ids, mask, pixels, tim_inputs=(tim_ids, tim_mask) if itm else None)
                vo = model.dual_encoder.vision_model(pixel_values=pixels)
            k = f"{fusion}.fwd{B}."
            out.update({k + "seed_x": seed_x, k + "ids": ids.numpy(), k + "mask": mask.numpy(), k + "onehot": onehot.numpy(), k + "out_cls": out_cls.numpy(),
                        k + "logits_per_text": lpt.numpy(), k + "mm_features": feats.numpy(), k + "vit_last_hidden_post0": vo.last_hidden_state[0].numpy(),
                        k + "vit_pooler_post0": vo.pooler_output[0].numpy()})
            if itm:
                out.update({k + "tim_ids": tim_ids.numpy(), k + "tim_mask": tim_mask.numpy(), k + "lbl_tim": lbl_tim.numpy(), k + "out_tim": out_tim.numpy()})
            print(tag, fusion, "fwd", B, "out_cls", out_cls.flatten()[:3].tolist(), "positive", round((feats > 0).float().mean().item(), 3))
        if fusion == "attention":          # the frozen tower under model.train(): two forwards of the same input differ
            model.train()
            px = O.synthetic_batch(cfg, 4, T, FWD[4], True)[2]
            torch.manual_seed(5)
            with torch.no_grad():
                a = model.dual_encoder.vision_model(pixel_values=px).pooler_output
                b = model.dual_encoder.vision_model(pixel_values=px).pooler_output
            out["stochastic.diff"] = (a - b).abs().max().item()
            assert out["stochastic.diff"] > 0
            print(tag, "train-mode tower, two forwards differ by", out["stochastic.diff"])
        # ---- training cases: drop path 0, dropout off, the reference's own losses
        with tempfile.TemporaryDirectory() as tmp:
            model = build_reference_model(ref_config, cfg0, txt_name, tmp, 0.0, 0.0)
        load_params(model, P)
        model.train()
        ids, mask, pixels, onehot = O.synthetic_batch(cfg0, TRAIN_B, T, TRAIN_SEED, True)
        np.random.seed(30)
        tim_ids, tim_mask, lbl_tim = O.prepare_itm_inputs(ids, mask)
        k = f"{fusion}.train."
        out.update({k + "B": TRAIN_B, k + "seed_x": TRAIN_SEED, k + "ids": ids.numpy(), k + "mask": mask.numpy(), k + "onehot": onehot.numpy(),
                    k + "class_weight": w.numpy(), k + "beta_itc": 0.1, k + "beta_itm": 0.1, k + "tim_ids": tim_ids.numpy(), k + "tim_mask": tim_mask.numpy(),
                    k + "lbl_tim": lbl_tim.numpy()})
        mixes = {"plain": (False, False), "itc": (True, False)}
        if fusion == "attention":
            mixes.update(itm=(False, True), itcitm=(True, True))
        for mix, (itc, itm) in mixes.items():
            model.zero_grad(set_to_none=True)
            o, lpt, ot, _, feats = model(ids, mask, pixels, tim_inputs=(tim_ids, tim_mask) if itm else None)
            label = onehot.type_as(o)                                # mm_late.py:471
            lc = loss_fn(o, label)
            if itc and itm:                                          # mm_late.py:473-487
                loss = (1 - 0.2) * lc + 0.1 * ref_utils.clip_loss(lpt) + 0.1 * tim_loss_fn(ot, lbl_tim)
            elif itc:
                loss = (1 - 0.1) * lc + 0.1 * ref_utils.clip_loss(lpt)
            elif itm:
                loss = (1 - 0.1) * lc + 0.1 * tim_loss_fn(ot, lbl_tim)
            else:
                loss = lc
            loss.backward()
            m = f"{fusion}.{mix}."
            out[m + "loss"] = loss.item()
            out[m + "out_cls"] = o.detach().numpy()
            out[m + "mm_features"] = feats.detach().numpy()
            if itm:
                out[m + "out_tim"] = ot.detach().numpy()
            G = grads_by_ref_key(model, WATCH)
            inv = {to_hf5_key(q): q for q in P}
            out[m + "grad_none"] = np.array(sorted(inv[n] for n, q in model.named_parameters() if q.requires_grad and q.grad is None))
            assert all(q.grad is None for n, q in model.named_parameters() if "vision_model" in n)
            for name in WATCH:
                g = G.get(name)
                if g is None:
                    continue
                out[m + f"gnorm.{name}"] = g.norm().item()
                if name.endswith("word_embeddings.weight"):
                    touched = torch.unique(ids)[:6]
                    out[m + f"gslice.{name}"] = g[touched][:, :48].numpy()
                    out[m + f"gslice_rows.{name}"] = touched.numpy()
                elif g.dim() == 2:
                    out[m + f"gslice.{name}"] = g[:8, :48].numpy()
                else:
                    out[m + f"gslice.{name}"] = g.flatten()[:64].numpy()
            print(tag, fusion, mix, "loss", loss.item(), "grad None:", len(out[m + "grad_none"]))
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= 784 * 1024, os.path.getsize(path)
    print(tag, os.path.getsize(path), "bytes")


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    rc = install_shim()
    tiny = dict(hidden=128, heads=2, inter=256, layers_txt=2, layers_img=2, vocab=1000, image=64, patch=16, img_kind="beit")
    case("beit_small_xlmr", dict(tiny, max_pos=130, num_labels=3), "bernice", 0, rc)
    case("beit_small_bert", dict(tiny, max_pos=512, type_vocab=2, txt_kind="bert", pad_id=0, ln_eps_txt=1e-12, num_labels=2), "bert", 1, rc)


if __name__ == "__main__":
    main()
