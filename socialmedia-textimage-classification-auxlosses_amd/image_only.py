"""Drop-in for the reference's image-only model and trainer (models/image_only.py, `vit` branch), backed by libmmhip.so.

  ViTClassifier    HF ViTForImageClassification -- ViT without a pooler, classifier(layernorm(x)[:, 0, :]) -- what the reference's
                   AutoModelForImageClassification.from_pretrained(dir, num_labels) builds (image_only.py:151).  forward(pixel_values) returns an
                   object with `.logits`, state_dict keys are those of transformers 4.25.1 (vit.embeddings.*, vit.encoder.layer.N.*,
                   vit.layernorm.*, classifier.*).  Forward and backward run the trainable image tower of the HIP engine (include/mmhip.h: mmhip_img_*).
  ImageModel       same role as reference models/image_only.py:122-317 (load_data, train, eval, the return dictionaries), with a fused step:
                   forward + loss + backward + AdamW on flat buffers in one native call.

Nothing random happens in a step: the checkpoint's tower dropouts are 0.0 and the reference never applies --dropout on this branch.  The reference
calls model.train() once before the epoch loop and its eval() leaves the model in eval mode for the rest of the run (image_only.py:187, 267); with
every dropout at 0 the two modes compute the same thing, so there is nothing to reproduce.  AdamW takes every parameter in one group with the same
weight decay, LayerNorm weights and biases included (utils.get_optimizer_params).
What this family shares with the text-only one -- the engine plumbing, the autograd edge, the trainer's steps, epoch loop and evaluation -- is
one_tower.py.  beit, deit, resnet50 / resnet152, conv_att and feature_extract are not part of this build.  There is no CPU / eager fallback.
"""
import types

import torch

from . import _lib
from . import dist as mmdist
from .config import IMAGE_ARCH, MODEL_DIR_DICT
from .engine_module import GuardedEngineModule
from .mm_late import _vit_key_to_ref
from .one_tower import OneTowerModule, OneTowerTrainer, tower_abi


def default_img_arch():
    a = dict(hidden=768, heads=12, inter=3072, layers=12, p_hidden=0.0, p_attn=0.0)
    a.update({k: v for k, v in IMAGE_ARCH["vit"].items() if k in ("image", "patch", "ln_eps_img")})
    return a


class ViTClassifier(OneTowerModule, GuardedEngineModule):
    """Keyword-only extras are additive, as in the other front ends: `arch` overrides (layer count, image size ... for tests), `dtype`
    ('bf16' | 'f16' | 'bf16x3'), `max_posts` (capacity), `device`, `seed` (of the random initialisation), `backward_products` (bf16x3 only)."""

    _family, _what, _ABI = "img", "image-only", tower_abi("img")
    _Config, _capacity_names = _lib.ImgConfig, ("max_posts",)

    def __init__(self, model_dir, num_labels, *, arch=None, dtype="bf16", max_posts=16, device=None, seed=0, backward_products=None):
        super().__init__()
        self._build(model_dir, num_labels, default_img_arch(), arch, dtype, (max_posts,), device, seed, backward_products)

    @staticmethod
    def _arch_from_hf(cfg, a):
        return dict(hidden=cfg.get("hidden_size", 768), heads=cfg.get("num_attention_heads", 12), inter=cfg.get("intermediate_size", 3072),
                    layers=cfg["num_hidden_layers"], image=cfg.get("image_size", 224), patch=cfg.get("patch_size", 16),
                    ln_eps_img=cfg.get("layer_norm_eps", 1e-12), p_hidden=cfg.get("hidden_dropout_prob", 0.0),
                    p_attn=cfg.get("attention_probs_dropout_prob", 0.0))

    @staticmethod
    def _cfg_keywords(a):
        return dict(image=a["image"], patch=a["patch"], ln_eps=a["ln_eps_img"])

    def _init_weights(self):
        """HF ViT initialisation: normal(0, 0.02) cut at two sigma for the Linears, the patch convolution, the position table and the CLS token, zero
        biases, unit LayerNorm weights (the classifier is a ViT Linear too: ViTPreTrainedModel._init_weights)"""
        g = torch.Generator(device=self.device_).manual_seed(self._seed_base)
        with torch.no_grad():
            for inf in self._infos:
                n, p = inf["name"], inf["param"]
                if "layernorm" in n and n.endswith(".weight"):
                    p.fill_(1.0)
                elif n.endswith(".bias"):
                    p.zero_()
                else:
                    p.normal_(0.0, 0.02, generator=g).clamp_(-0.04, 0.04)

    def _load_checkpoint(self, sd):
        """a ViTModel / ViTForImageClassification state dict of either key generation: transformers 4.25.1 (vit.encoder.layer.N.attention.attention.query ...)
        or >= 5 (vit.layers.N.attention.q_proj ...); a classifier of another width (the checkpoint's 1000 ImageNet classes) stays newly
        initialised, as from_pretrained(num_labels=...) leaves it"""
        own = {inf["name"]: inf["param"] for inf in self._infos}
        with torch.no_grad():
            for k, v in sd.items():
                if k.startswith("classifier."):
                    name = k
                else:
                    name = "vit." + _vit_key_to_ref(k[4:] if k.startswith("vit.") else k)
                if name in own and tuple(own[name].shape) == tuple(v.shape):
                    own[name].copy_(v.to(own[name].device, torch.float32))

    def _inputs(self, pixels):
        px = pixels.to(self.device_, torch.float32)
        if px.dim() == 5 and px.shape[1] == 1:          # loader items carry [1, 3, S, S]
            px = px[:, 0]
        if px.dim() == 3:
            px = px.unsqueeze(0)
        S = self.arch["image"]
        if px.dim() != 4 or tuple(px.shape[1:]) != (3, S, S):
            raise ValueError(f"image-only forward: pixel_values {tuple(pixels.shape)}, expected [B, 3, {S}, {S}]")
        return (px.contiguous(),)

    def _forward_args(self, seed, px):
        self._last = dict(B=px.shape[0])
        return [_lib.ptr(px), px.shape[0], int(self.training)]

    def _step_args(self, seed, onehot, cw, px):
        self._last = dict(B=px.shape[0])
        return [_lib.ptr(px), _lib.ptr(onehot), _lib.ptr(cw), px.shape[0]]

    def forward(self, pixel_values):
        """-> an object with `.logits` [B, num_labels] (the reference reads `output.logits`, image_only.py:209-210)"""
        return types.SimpleNamespace(logits=self._logits(pixel_values))


# =====================================================================================================================
class ImageModel(OneTowerTrainer):
    """reference models/image_only.py:122-317.  A step takes `pixels, onehot, class_weight, lr, weight_decay, step`."""

    _overflow_note = "non-finite gradient element(s) were dropped"
    _eval_line = "test loss: {:.4f} test acc: {:.4f}\n"

    def __init__(self, batch_size, num_labels, model_name, conv_att=False, feature_extract=False, max_grad_norm=None, **model_kw):
        self._refuse_grad_clip_under_dp(max_grad_norm, mmdist.world_size())
        if model_name != "vit":
            raise NotImplementedError(f"image model {model_name!r}: the image-only path builds `vit` (HF ViTForImageClassification); beit, deit and "
                                      "the resnets are not part of this build")
        if conv_att or feature_extract:
            raise NotImplementedError("conv_att / feature_extract belong to the reference's CNN models, which are not part of this build")
        if mmdist.world_size() > 1:
            raise NotImplementedError("the image-only trainer is single-process: data-parallel training of this path is not implemented "
                                      f"(world size {mmdist.world_size()}); launch one process")
        self.batch_size, self.num_labels, self.model_name = batch_size, num_labels, model_name
        self.cnn = False
        self.model_dir = MODEL_DIR_DICT[model_name]
        model_kw.setdefault("max_posts", batch_size)
        self.model = ViTClassifier(self.model_dir, num_labels, **model_kw)
        self.device = self.model.device_
        self.set_max_grad_norm(max_grad_norm)

    # ---- data
    def load_data(self, data, img_file_fmt, testing=False, task_name=None):
        """reference :160-177 -> (train_loader, val_loader, test_loader, class_weights); like the reference's, the training loader is not shuffled"""
        from .datasets import ImgOnly_Dataset, prepare_data
        tr, ytr, va, yva, te, yte, w = prepare_data(data, self.num_labels, testing=testing)
        mk = lambda df, y: ImgOnly_Dataset(df.tweet_id.values, y, None, img_file_fmt, task_name=task_name, image=self.model.arch["image"])
        dl = lambda ds: torch.utils.data.DataLoader(ds, batch_size=self.batch_size)
        return dl(mk(tr, ytr)), dl(mk(va, yva)), dl(mk(te, yte)), w

    def _item(self, dl):
        return (dl["pixel_values"],), dl["labels"]
