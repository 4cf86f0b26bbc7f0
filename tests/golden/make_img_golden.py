#!/usr/bin/env python3
"""Golden vectors of the image-only model, made with the REFERENCE's own code path (models/image_only.py:151 -- AutoModelForImageClassification
.from_pretrained(dir, num_labels) --, utils.get_optimizer_params, torch.optim.AdamW, nn.CrossEntropyLoss(weight); needs the reference checkout next
to this tree, CPU only).  The shim is make_golden.py's, imported unchanged.

Writes tests/golden/img_small_vit.npz: 2 layers, 192 px (145 tokens), B = 2, 3 labels -- the pixels as uint8 (pixel = u8 / 127.5 - 1), eval-mode
logits, train-mode logits and loss under class weights, and for every parameter (tests/img_ref.py pick: the first 2 rows of matrices of more than 8
rows; rows 0, 1, 2 and the last of the position table) the gradient and the value after one AdamW step; the sorted state-dict keys under their
transformers 4.25.1 names.  Nothing of the reference is copied: the file is data.
Run:  python tests/golden/make_img_golden.py
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
import img_ref as R  # noqa: E402


def to_installed(k):
    """4.25.1 reference key -> the installed transformers' key (>= 5: vit.layers.N.attention.q_proj ...; older: unchanged)"""
    import transformers
    if int(transformers.__version__.split(".")[0]) < 5:
        return k
    k = k.replace("vit.encoder.layer.", "vit.layers.")
    k = k.replace("attention.attention.query", "attention.q_proj").replace("attention.attention.key", "attention.k_proj")
    k = k.replace("attention.attention.value", "attention.v_proj").replace("attention.output.dense", "attention.o_proj")
    return k.replace("intermediate.dense", "mlp.fc1").replace("output.dense", "mlp.fc2")


def case(tag, image, B):
    import utils as ref_utils
    import image_only as ref_img  # noqa: F401  (the module whose `vit` branch this restates: AutoModelForImageClassification.from_pretrained)
    from transformers import AutoModelForImageClassification, ViTConfig, ViTForImageClassification
    cfg = R.oracle_cfg(image=image)
    P = R.make_params(cfg, 0)
    with tempfile.TemporaryDirectory() as d:
        # (a saved bare ViTModel does not load into the classifier under transformers 5: its layers come up newly initialised)
        ViTForImageClassification(ViTConfig(num_hidden_layers=cfg.layers_img, image_size=image, num_labels=cfg.num_labels)).save_pretrained(d)
        model = AutoModelForImageClassification.from_pretrained(d, num_labels=cfg.num_labels)          # image_only.py:151
    assert model.config.hidden_dropout_prob == 0.0 and model.config.attention_probs_dropout_prob == 0.0
    mapped = {to_installed(k): v for k, v in P.items()}
    assert set(mapped) == set(model.state_dict())
    model.load_state_dict(mapped)
    sd = model.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in mapped.items())
    u8, px, onehot = R.pixels_u8(cfg, B, 7)
    model.eval()
    with torch.no_grad():
        logits = model(pixel_values=px).logits
    model.train()                                                  # image_only.py:187
    w = torch.tensor([1.0, 2.0, 0.5])
    loss_fn = torch.nn.CrossEntropyLoss(weight=w)                  # run_img.py:56
    lr, wd = 1e-3, 0.01
    opt = torch.optim.AdamW(ref_utils.get_optimizer_params(model.named_parameters(), wd, lr), lr=lr)      # image_only.py:182-184
    opt.zero_grad()
    out = model(pixel_values=px).logits
    loss = loss_fn(out, onehot.type_as(out))                       # image_only.py:213-215
    loss.backward()
    named = dict(model.named_parameters())
    data = dict(cfg=np.array(repr(O.asdict(cfg))), B=B, pixels_u8=u8.numpy(), onehot=onehot.numpy(), class_weight=w.numpy(), lr=lr, weight_decay=wd,
                logits=logits.numpy(), train_logits=out.detach().numpy(), loss=loss.item(), watch=np.array(sorted(P)), keys=np.array(sorted(P)))
    for k in sorted(P):
        data["grad." + k] = R.pick(k, named[to_installed(k)].grad).numpy()
    opt.step()
    for k in sorted(P):
        data["after." + k] = R.pick(k, named[to_installed(k)].detach()).numpy()
    path = os.path.join(HERE, f"{tag}.npz")
    np.savez_compressed(path, **data)
    print(tag, "logits", logits.flatten()[:3].tolist(), "loss", loss.item(), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    install_shim()
    sys.modules["torchmetrics.classification"].BinaryF1Score = object      # image_only.py:15 imports it; the stub has no such name
    case("img_small_vit", 192, 2)
