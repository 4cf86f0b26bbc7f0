"""fp32 restatement of the reference's image-only model (models/image_only.py `vit` branch: HF ViTForImageClassification), composed from the pinned
oracle: logits = classifier(vit_forward(...)[0][:, 0, :]) -- ViT without a pooler, the final LayerNorm inside vit_forward's first return value.
oracle.mm_oracle is imported, not modified; its vit_forward wants a pooler, whose output is unused here: a zero one is supplied."""
import torch
import torch.nn.functional as F

from oracle import mm_oracle as O

VM_REF, VM_ORACLE = "vit.", "dual_encoder.vision_model."


def oracle_cfg(layers=2, image=192, num_labels=3, **kw):
    base = dict(layers_txt=0, layers_img=layers, image=image, num_labels=num_labels)
    base.update(kw)
    return O.OracleConfig(**base)


def param_shapes(cfg):
    """state-dict keys (transformers 4.25.1) and shapes of ViTForImageClassification"""
    s = {VM_REF + k[len(VM_ORACLE):]: v for k, v in O.param_shapes(cfg).items() if k.startswith(VM_ORACLE) and ".pooler." not in k}
    s["classifier.weight"], s["classifier.bias"] = (cfg.num_labels, cfg.hidden), (cfg.num_labels,)
    return s


def make_params(cfg, seed=0):
    """O.make_param(name, shape, seed) under the reference's keys"""
    return {k: O.make_param(k, shp, seed) for k, shp in param_shapes(cfg).items()}


def forward(P, pixels, cfg):
    """logits [B, C]"""
    Q = {VM_ORACLE + k[len(VM_REF):]: v for k, v in P.items() if k.startswith(VM_REF)}
    Q[VM_ORACLE + "pooler.dense.weight"] = torch.zeros(cfg.hidden, cfg.hidden)
    Q[VM_ORACLE + "pooler.dense.bias"] = torch.zeros(cfg.hidden)
    x, _ = O.vit_forward(Q, pixels, cfg)
    return F.linear(x[:, 0], P["classifier.weight"], P["classifier.bias"])


def loss_and_grads(P, pixels, onehot, weight, cfg):
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    logits = forward(Pg, pixels, cfg)
    loss = O.cls_loss(logits, onehot, weight)
    loss.backward()
    return logits.detach(), loss.detach(), {k: v.grad for k, v in Pg.items()}


def adamw(P, G, M, V, step, lr, wd):
    """torch.optim.AdamW, one group: every parameter with the same weight decay (utils.get_optimizer_params), in place"""
    for k, g in G.items():
        O.adamw_step(P[k], g, M[k], V[k], step, lr, wd)


def pixels_u8(cfg, B, seed):
    """a synthetic batch whose pixels are exactly representable as uint8 (pixel = u8 / 127.5 - 1): what the golden stores; -> (u8, pixels, onehot)"""
    _, _, px, onehot = O.synthetic_batch(O.OracleConfig(vocab=500, image=cfg.image, num_labels=cfg.num_labels), B, 8, seed)
    u8 = torch.round((px + 1) * 127.5).clamp(0, 255).to(torch.uint8)
    return u8, from_u8(u8), onehot


def from_u8(u8):
    return u8.float() / 127.5 - 1


def pick(name, x):
    """the rows of a watched tensor the golden keeps: the first 2 rows of matrices of more than 8 rows; rows 0, 1, 2 and the last of the position table"""
    if name == "vit.embeddings.position_embeddings":
        return x[0, [0, 1, 2, x.shape[1] - 1]]
    return x[:2] if x.dim() >= 2 and x.shape[0] > 8 else x
