"""fp32 restatement of the reference's text-only modules (models/text_only.py BERT / BERNICE), composed from the pinned oracle:
logits = linear(dropout(text_forward(...)[:, 0, :])).  oracle.mm_oracle is imported, not modified."""
import torch
import torch.nn.functional as F

from oracle import mm_oracle as O

TM_REF, TM_ORACLE = "bert_model.", "dual_encoder.text_model."


def oracle_cfg(layers=2, vocab=500, num_labels=3, kind="xlmr", **kw):
    base = dict(layers_txt=layers, layers_img=0, vocab=vocab, num_labels=num_labels)
    base.update(dict(txt_kind="xlmr", max_pos=130, type_vocab=1, pad_id=1, ln_eps_txt=1e-5) if kind == "xlmr" else
                dict(txt_kind="bert", max_pos=128, type_vocab=2, pad_id=0, ln_eps_txt=1e-12))
    base.update(kw)
    return O.OracleConfig(**base)


def param_shapes(cfg):
    """state-dict keys and shapes of the reference modules (without the position_ids buffer)"""
    s = {TM_REF + k[len(TM_ORACLE):]: v for k, v in O.param_shapes(cfg).items() if k.startswith(TM_ORACLE)}
    s["linear.weight"], s["linear.bias"] = (cfg.num_labels, cfg.hidden), (cfg.num_labels,)
    return s


def make_params(cfg, seed=0):
    """the oracle's deterministic text-tower weights under the reference's keys; linear.* drawn with make_param"""
    return {k: O.make_param(TM_ORACLE + k[len(TM_REF):] if k.startswith(TM_REF) else k, shp, seed) for k, shp in param_shapes(cfg).items()}


def trainable(name):
    return ".pooler." not in name          # computed by the reference, never consumed: grad is None


def forward(P, ids, mask, type_ids, cfg, drop=None):
    """logits [B, C].  Non-zero token types (BERT, positions independent of the ids): the oracle's tower always adds type row 0, so each
    slot gets its own word row  word[id] + type[t] - type[0]  -- the same sum, differentiable into both tables."""
    Q = {TM_ORACLE + k[len(TM_REF):]: v for k, v in P.items() if k.startswith(TM_REF)}
    if type_ids is not None and cfg.type_vocab > 1:
        assert cfg.txt_kind == "bert"
        w, ty = Q[TM_ORACLE + "embeddings.word_embeddings.weight"], Q[TM_ORACLE + "embeddings.token_type_embeddings.weight"]
        Q[TM_ORACLE + "embeddings.word_embeddings.weight"] = (w[ids] + ty[type_ids] - ty[0]).reshape(-1, w.shape[1])
        ids = torch.arange(ids.numel()).view_as(ids)
    x, _ = O.text_forward(Q, ids, mask, cfg, drop)
    drop = drop or O.Dropout("none")
    return F.linear(drop(x[:, 0].contiguous(), cfg.p_head, O.STREAM_HEAD, 0), P["linear.weight"], P["linear.bias"])


def loss_and_grads(P, ids, mask, type_ids, onehot, weight, cfg, drop=None):
    Pg = {k: v.clone().requires_grad_(trainable(k)) for k, v in P.items()}
    logits = forward(Pg, ids, mask, type_ids, cfg, drop)
    loss = O.cls_loss(logits, onehot, weight)
    loss.backward()
    return logits.detach(), loss.detach(), {k: v.grad for k, v in Pg.items()}


def adamw(P, G, M, V, step, lr, wd):
    """torch.optim.AdamW over the parameters that have a gradient (torch skips grad is None), in place"""
    for k, g in G.items():
        if g is not None:
            O.adamw_step(P[k], g, M[k], V[k], step, lr, wd)
