#!/usr/bin/env python3
"""Golden vectors of the text-only models, made by running the REFERENCE's own code (models/text_only.py BERNICE / BERT; needs the reference
checkout next to this tree, CPU only).  The shim and the random-init directory recipe are make_golden.py's, imported unchanged.

Writes tests/golden/txt_small_xlmr.npz and txt_small_bert.npz: 2 layers, vocab 500, B = 4, T = 32, padded rows, 3 labels (BERT: non-zero token types
on some tokens) -- inputs, eval-mode logits, the dropout-off train-mode loss under class weights, gradients of a watched set and the watched
parameters after one torch.optim.AdamW step built with the reference's get_optimizer_params.  Matrices with more than 8 rows are stored as listed
rows only ("rows.<name>"): EVERY word row that occurs for the word table's gradient, 8 occurring rows for the position table, the first 2 rows of the
dense weights; after the step the word table keeps the first 8 of its rows ("arows.<name>").  Nothing of the reference is copied: the files are data.
Run:  python tests/golden/make_txt_golden.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))
from make_golden import install_shim, O  # noqa: E402
import txt_ref as R  # noqa: E402

WATCH = ["linear.weight", "linear.bias", "bert_model.embeddings.LayerNorm.weight", "bert_model.embeddings.LayerNorm.bias",
         "bert_model.embeddings.position_embeddings.weight", "bert_model.embeddings.word_embeddings.weight",
         "bert_model.embeddings.token_type_embeddings.weight",
         "bert_model.encoder.layer.0.attention.self.query.weight", "bert_model.encoder.layer.0.attention.self.key.bias",
         "bert_model.encoder.layer.0.attention.self.value.weight", "bert_model.encoder.layer.0.attention.output.dense.weight",
         "bert_model.encoder.layer.0.attention.output.LayerNorm.weight", "bert_model.encoder.layer.0.intermediate.dense.weight",
         "bert_model.encoder.layer.0.intermediate.dense.bias", "bert_model.encoder.layer.1.output.dense.weight",
         "bert_model.encoder.layer.1.output.LayerNorm.bias", "bert_model.encoder.layer.1.attention.self.query.weight",
         "bert_model.pooler.dense.weight"]


def build(ref_config, cfg, kind, tmp, p):
    from transformers import XLMRobertaConfig, XLMRobertaModel, BertConfig, BertModel
    d = os.path.join(tmp, kind)
    if kind == "xlmr":
        XLMRobertaModel(XLMRobertaConfig(vocab_size=cfg.vocab, max_position_embeddings=cfg.max_pos, type_vocab_size=1, layer_norm_eps=cfg.ln_eps_txt,
                                         num_hidden_layers=cfg.layers_txt, hidden_dropout_prob=p, attention_probs_dropout_prob=p, pad_token_id=1,
                                         bos_token_id=0, eos_token_id=2)).save_pretrained(d)
    else:
        BertModel(BertConfig(vocab_size=cfg.vocab, max_position_embeddings=cfg.max_pos, type_vocab_size=2, num_hidden_layers=cfg.layers_txt,
                             hidden_dropout_prob=p, attention_probs_dropout_prob=p)).save_pretrained(d)
    import text_only as ref_txt
    return (ref_txt.BERNICE if kind == "xlmr" else ref_txt.BERT)(d, cfg.num_labels, dropout=p)


def load(model, P):
    sd = model.state_dict()
    missing = [k for k in sd if k not in P and not k.endswith("position_ids") and not k.endswith("token_type_ids")]
    assert not missing and not [k for k in P if k not in sd], missing
    model.load_state_dict(P, strict=False)


def rows_of(name, ids, pos, cfg):
    if name.endswith("word_embeddings.weight"):
        return torch.unique(ids)
    if name.endswith("position_embeddings.weight"):
        return torch.unique(pos)[:8]
    return torch.arange(0, 2)


def case(tag, kind, ref_config):
    import utils as ref_utils
    cfg = R.oracle_cfg(kind=kind, p_hidden=0.0, p_attn=0.0, p_head=0.0)
    B, T = 4, 32
    P = R.make_params(cfg, 0)
    ids, mask, _, onehot = O.synthetic_batch(O.OracleConfig(**{**O.asdict(cfg), "image": 16}), B, T, 7, True)
    tt = None
    if kind == "bert":
        tt = torch.zeros(B, T, dtype=torch.int64)
        tt[:, T // 3:] = 1
        tt[1] = 0
        tt = tt * mask
    call = (lambda m: m(ids, mask)) if kind == "xlmr" else (lambda m: m(ids, mask, tt))
    with tempfile.TemporaryDirectory() as tmp:
        model = build(ref_config, cfg, kind, tmp, 0.0)
    load(model, P)
    model.eval()
    with torch.no_grad():
        logits = call(model)
    model.train()
    w = torch.tensor([1.0, 2.0, 0.5])
    loss_fn = torch.nn.CrossEntropyLoss(weight=w)                 # run_txt.py:54
    lr, wd = 1e-3, 0.01
    opt = torch.optim.AdamW(ref_utils.get_optimizer_params(model.named_parameters(), wd, lr), lr=lr)      # text_only.py:128-130
    opt.zero_grad()
    out = call(model)
    loss = loss_fn(out, onehot.type_as(out))                      # text_only.py:156,161
    loss.backward()
    named = dict(model.named_parameters())
    pos = O.text_position_ids(ids, cfg)
    data = dict(cfg=np.array(repr(O.asdict(cfg))), B=B, T=T, ids=ids.numpy(), mask=mask.numpy(), onehot=onehot.numpy(), class_weight=w.numpy(),
                lr=lr, weight_decay=wd, logits=logits.numpy(), train_logits=out.detach().numpy(), loss=loss.item(), watch=np.array(WATCH),
                keys=np.array(sorted(model.state_dict())))
    if tt is not None:
        data["token_type_ids"] = tt.numpy()
    sel = {}
    for k in WATCH:
        g = named[k].grad
        data["nograd." + k] = g is None
        sel[k] = rows_of(k, ids, pos, cfg) if named[k].dim() == 2 and named[k].shape[0] > 8 else None
        if sel[k] is not None:
            data["rows." + k] = sel[k].numpy()
        if g is not None:
            data["grad." + k] = (g if sel[k] is None else g[sel[k]]).numpy()
    opt.step()
    for k in WATCH:
        v = named[k].detach()
        rows = sel[k]
        if rows is not None and rows.numel() > 8:
            rows = rows[:8]
            data["arows." + k] = rows.numpy()
        data["after." + k] = (v if rows is None else v[rows]).numpy()
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **data)
    print(tag, "logits", logits.flatten()[:3].tolist(), "loss", loss.item(), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    rc = install_shim()
    case("txt_small_xlmr", "xlmr", rc)
    case("txt_small_bert", "bert", rc)
