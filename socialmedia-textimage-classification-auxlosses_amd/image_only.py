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
beit, deit, resnet50 / resnet152, conv_att and feature_extract are not part of this build.  There is no CPU / eager fallback.
"""
import logging
import os
import types

import numpy as np
import torch

from . import _lib
from . import dist as mmdist
from .config import IMAGE_ARCH, MODEL_DIR_DICT, metric_names
from .engine_module import EngineModule, FlatTrainer, _read_hf_dir, merge_ranges
from .mm_late import _vit_key_to_ref
from .utils import agg_metrics_val

logger = logging.getLogger(__name__)


def default_img_arch():
    a = dict(hidden=768, heads=12, inter=3072, layers=12, p_hidden=0.0, p_attn=0.0)
    a.update({k: v for k, v in IMAGE_ARCH["vit"].items() if k in ("image", "patch", "ln_eps_img")})
    return a


class _ImgFunction(torch.autograd.Function):
    """autograd edge around the engine so that the reference's loss.backward() (image_only.py:217) works on the returned logits"""

    @staticmethod
    def forward(ctx, model, pixels, *params):
        out = model._engine_forward(pixels)
        ctx.model, ctx.token = model, model._fwd_token
        return out

    @staticmethod
    def backward(ctx, d_logits):
        model = ctx.model
        if ctx.token != model._fwd_token:
            raise RuntimeError("image-only model: backward() after another forward(); the engine keeps one set of activations")
        return (None,) * 2 + tuple(model._engine_backward_autograd(d_logits))


class ViTClassifier(EngineModule):
    """Keyword-only extras are additive, as in the other front ends: `arch` overrides (layer count, image size ... for tests), `dtype`
    ('bf16' | 'f16' | 'bf16x3'), `max_posts` (capacity), `device`, `seed` (of the random initialisation), `backward_products` (bf16x3 only)."""

    _ABI = dict(create="mmhip_img_create", destroy="mmhip_img_destroy", param_count="mmhip_img_param_count", param_info_at="mmhip_img_param_info_at",
                workspace_bytes="mmhip_img_workspace_bytes", num_stages="mmhip_num_backward_stages", stage_grad_range="mmhip_stage_grad_range")

    def __init__(self, model_dir, num_labels, *, arch=None, dtype="bf16", max_posts=16, device=None, seed=0, backward_products=None):
        super().__init__()
        if not torch.cuda.is_available():
            raise _lib.MMHipError("the image-only model needs an MI355X (gfx950) GPU: the HIP path has no CPU fallback")
        self.num_labels = int(num_labels)
        self.device_ = torch.device(device if device is not None else f"cuda:{int(os.environ.get('LOCAL_RANK', 0))}")
        a = default_img_arch()
        cfg, sd = _read_hf_dir(model_dir or "")
        if cfg:
            a.update(hidden=cfg.get("hidden_size", 768), heads=cfg.get("num_attention_heads", 12), inter=cfg.get("intermediate_size", 3072),
                     layers=cfg["num_hidden_layers"], image=cfg.get("image_size", 224), patch=cfg.get("patch_size", 16),
                     ln_eps_img=cfg.get("layer_norm_eps", 1e-12), p_hidden=cfg.get("hidden_dropout_prob", 0.0),
                     p_attn=cfg.get("attention_probs_dropout_prob", 0.0))
        a.update(arch or {})
        self.arch, self.dtype_name = a, dtype
        if backward_products is not None and (dtype != "bf16x3" or int(backward_products) not in (1, 2, 3)):
            raise ValueError("backward_products is 1, 2 or 3 and belongs to dtype='bf16x3'")
        self.backward_products = None if backward_products is None else int(backward_products)
        self._loss_scale = 0.0
        self._cfg_kw = dict(hidden=a["hidden"], heads=a["heads"], inter=a["inter"], layers=a["layers"], image=a["image"], patch=a["patch"],
                            ln_eps=a["ln_eps_img"], num_labels=self.num_labels, p_hidden=a["p_hidden"], p_attn=a["p_attn"],
                            dtype={"bf16": _lib.BF16, "f16": _lib.F16, "bf16x3": _lib.BF16X3}[dtype])
        self._init_engine(int(seed) if seed is not None else int(torch.initial_seed()))
        self._create_engine(max_posts)
        self._init_weights()
        if sd is not None:
            self._load_checkpoint(sd)
        self._refresh_weights()

    # ------------------------------------------------------------------ engine / buffers
    def _config(self, max_posts):
        return _lib.ImgConfig(max_posts=int(max_posts), loss_scale=float(self._loss_scale), **self._cfg_kw)

    def _allocate_flats(self, h):
        n = _lib.lib().mmhip_img_numel(h)
        self._flat_train = torch.zeros(n, dtype=torch.float32, device=self.device_)
        self._flat_grad = torch.zeros(n, dtype=torch.float32, device=self.device_)
        return {1: self._flat_train}

    def _on_registered(self):
        # device words of every handle: include/mmhip.h mmhip_set_guard {non-finite counter, void-step flag}
        self._guard4 = torch.zeros(4, dtype=torch.int32, device=self.device_)
        self._nonfinite = self._guard4[:2]

    def _apply_setters(self, h):
        lib = _lib.lib()
        _lib.check(lib.mmhip_set_guard(h, _lib.ptr(self._nonfinite)), "set_guard")
        if self.backward_products is not None:
            _lib.check(lib.mmhip_set_backward_products(h, self.backward_products), "set_backward_products")

    def _bind(self, h):
        _lib.check(_lib.lib().mmhip_img_bind(h, _lib.ptr(self._flat_train), _lib.ptr(self._flat_grad), _lib.ptr(self._ws), self._ws.numel()), "img_bind")

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

    def _refresh_weights(self):
        _lib.check(_lib.lib().mmhip_img_refresh_weights(self._handle, _lib.stream_ptr()), "img_refresh_weights")
        self._weights_version = self._flat_train._version

    def _ensure(self, B):
        (cap_b,) = self._capacity
        if B > cap_b:
            self._create_engine(max(B, cap_b))
            self._refresh_weights()
        elif self._weights_version != self._flat_train._version:
            self._refresh_weights()        # parameters were modified in place (optimizer.step / load_state_dict)

    def _pixels(self, pixels):
        px = pixels.to(self.device_, torch.float32)
        if px.dim() == 5 and px.shape[1] == 1:          # loader items carry [1, 3, S, S]
            px = px[:, 0]
        if px.dim() == 3:
            px = px.unsqueeze(0)
        S = self.arch["image"]
        if px.dim() != 4 or tuple(px.shape[1:]) != (3, S, S):
            raise ValueError(f"image-only forward: pixel_values {tuple(pixels.shape)}, expected [B, 3, {S}, {S}]")
        return px.contiguous()

    def _engine_forward(self, pixels):
        px = self._pixels(pixels)
        B = px.shape[0]
        self._ensure(B)
        logits = torch.empty(B, self.num_labels, device=self.device_)
        _lib.check(_lib.lib().mmhip_img_forward(self._handle, _lib.ptr(px), B, int(self.training), _lib.ptr(logits), _lib.stream_ptr()), "img_forward")
        self._fwd_token += 1
        self._last = dict(B=B)
        return logits

    def active_ranges(self):
        """merged [begin, end) element ranges of the flat buffer that AdamW steps: all of it"""
        return merge_ranges((i["offset"], i["numel"]) for i in self._infos)

    def _engine_backward(self, d_logits=None):
        """gradient of the last forward into the flat gradient buffer (cleared first); d_logits None: the one mmhip_img_loss left in the handle"""
        self._zero_grad_state()
        if d_logits is not None:
            d_logits = d_logits.to(self.device_, torch.float32).contiguous()
        _lib.check(_lib.lib().mmhip_img_backward(self._handle, _lib.ptr(d_logits), _lib.stream_ptr()), "img_backward")
        self._grad_dirty = True

    def _engine_backward_autograd(self, d_logits):
        self._engine_backward(d_logits)
        return [self._flat_grad[inf["offset"]: inf["offset"] + inf["numel"]].view(inf["shape"]).clone() for inf in self._infos]

    def forward(self, pixel_values):
        """-> an object with `.logits` [B, num_labels] (the reference reads `output.logits`, image_only.py:209-210)"""
        if torch.is_grad_enabled() and any(i["param"].requires_grad for i in self._infos):
            logits = _ImgFunction.apply(self, pixel_values, *[i["param"] for i in self._infos])
        else:
            logits = self._engine_forward(pixel_values)
        return types.SimpleNamespace(logits=logits)


# =====================================================================================================================
class ImageModel(FlatTrainer):
    """reference models/image_only.py:122-317.  `train()` / `eval()` keep the reference's semantics and return dictionaries; the step is fused."""

    def __init__(self, batch_size, num_labels, model_name, conv_att=False, feature_extract=False, **model_kw):
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
        self._opt = None

    # ---- data
    def load_data(self, data, img_file_fmt, testing=False, task_name=None):
        """reference :160-177 -> (train_loader, val_loader, test_loader, class_weights); like the reference's, the training loader is not shuffled"""
        from .datasets import ImgOnly_Dataset, prepare_data
        tr, ytr, va, yva, te, yte, w = prepare_data(data, self.num_labels, testing=testing)
        mk = lambda df, y: ImgOnly_Dataset(df.tweet_id.values, y, None, img_file_fmt, task_name=task_name, image=self.model.arch["image"])
        dl = lambda ds: torch.utils.data.DataLoader(ds, batch_size=self.batch_size)
        return dl(mk(tr, ytr)), dl(mk(va, yva)), dl(mk(te, yte)), w

    # ---- optimizer state: one dense range, no word table
    def _moments(self):
        if self._opt is None:
            self._opt = (torch.zeros_like(self.model._flat_train), torch.zeros_like(self.model._flat_train))
        return self._opt

    def _adamw_ranges(self, ranges, lr, weight_decay, step, grad_scale=1.0):
        import ctypes as C
        m, lib = self.model, _lib.lib()
        em, ev = self._moments()
        at = lambda t, el: C.c_void_p(t.data_ptr() + el * 4)
        for b, e in ranges:
            _lib.check(lib.mmhip_adamw_guarded(at(m._flat_train, b), at(m._flat_grad, b), at(em, b), at(ev, b), e - b, lr, 0.9, 0.999, 1e-8,
                                               weight_decay, step, grad_scale, 1, _lib.stream_ptr(), _lib.ptr(m._nonfinite)), "adamw")

    def _labels(self, onehot, class_weight):
        onehot = onehot.to(self.device, torch.int64).contiguous()
        cw = None if class_weight is None else class_weight.to(self.device, torch.float32).contiguous()
        return onehot, cw

    # ---- one fused training step on device tensors -> (loss[1] device tensor, n_correct[1] device tensor)
    def train_step(self, pixels, onehot, class_weight, lr, weight_decay, step):
        m = self.model
        if not m.training:
            m.train()
        m._clean_grad()
        px = m._pixels(pixels)
        B = px.shape[0]
        m._ensure(B)
        em, ev = self._moments()
        onehot, cw = self._labels(onehot, class_weight)
        loss = torch.empty(1, device=self.device)
        ncorr = torch.empty(1, dtype=torch.int32, device=self.device)
        m._last = dict(B=B)
        _lib.check(_lib.lib().mmhip_img_train_step(m._handle, _lib.ptr(px), _lib.ptr(onehot), _lib.ptr(cw), B, _lib.ptr(em), _lib.ptr(ev), lr, 0.9, 0.999,
                                                   1e-8, weight_decay, step, _lib.ptr(loss), _lib.ptr(ncorr), _lib.stream_ptr()), "img_train_step")
        m._fwd_token += 1
        m._weights_version = m._flat_train._version          # the refresh inside the call keeps the 16-bit copies current
        return loss, ncorr

    # ---- the same step as separate calls (forward, loss, backward, AdamW): what the fused call is checked against
    def staged_step(self, pixels, onehot, class_weight, lr, weight_decay, step):
        m, lib = self.model, _lib.lib()
        if not m.training:
            m.train()
        m._clean_grad()
        m._engine_forward(pixels)
        onehot, cw = self._labels(onehot, class_weight)
        loss = torch.empty(1, device=self.device)
        ncorr = torch.empty(1, dtype=torch.int32, device=self.device)
        _lib.check(lib.mmhip_img_loss(m._handle, _lib.ptr(onehot), _lib.ptr(cw), _lib.ptr(loss), _lib.ptr(ncorr), _lib.stream_ptr()), "img_loss")
        m._engine_backward(None)
        self._adamw_ranges(m.active_ranges(), lr, weight_decay, step)
        m._grad_dirty = False
        m._refresh_weights()
        return loss, ncorr

    def check_overflow(self):
        n = int(self.model._nonfinite[0].item()) - getattr(self, "_nf_seen", 0)
        if n > 0:
            self._nf_seen = getattr(self, "_nf_seen", 0) + n
            if self.model.dtype_name != "f16":
                raise FloatingPointError(f"non-finite gradients met {n} times ({self.model.dtype_name}): the run has diverged")
            logger.warning("f16 gradient overflow: %d non-finite gradient element(s) were dropped on the device", n)
        return max(n, 0)

    def train(self, dataloader, val_dataloader, epochs, loss_fn=None, lr=1e-5, weight_decay=0.00025, te_dataloader=None, model_path=None,
              val_filename=None, te_filename=None, class_weight=None, log_every=50):
        """reference :179-258.  `loss_fn` is accepted for signature parity: the class weights it carries (nn.CrossEntropyLoss(weight=w),
        run_img.py:56) are what the fused step uses."""
        import pandas as pd
        class_weight = self._class_weight(loss_fn, class_weight)
        res_val, res_te, step = [], [], 0
        for epoch in range(epochs):
            print(epoch)
            for it, dl in enumerate(dataloader):
                step += 1
                loss, ncorr = self.train_step(dl["pixel_values"], dl["labels"], class_weight, lr, weight_decay, step)
                if log_every and it % log_every == 0:          # the reference syncs and prints every step (:222-229)
                    self.check_overflow()
                    n = dl["labels"].shape[0]
                    print(f"Got {int(ncorr.item())} / {n} with accuracy {float(ncorr.item()) / n * 100:.2f} loss {loss[0].item():.4f}")
            for loader, store, fname, tag in ((val_dataloader, res_val, val_filename, "val"), (te_dataloader, res_te, te_filename, "test")):
                if loader is None:
                    continue
                print(tag)
                r = self.eval(loader, class_weight=class_weight)
                r["epoch"] = epoch
                store.append(r)
                if fname is not None and (epoch % 2 == 0 or epoch == epochs - 1):
                    pd.DataFrame(agg_metrics_val(store, metric_names, self.num_labels)).to_csv(fname, index=False)
                    logger.info("%s saved!", fname)
        if model_path is not None:
            self.save_model(model_path)
            logger.info("%s saved", model_path)

    def eval(self, dataloader, loss_fn=None, class_weight=None):
        """reference :260-317 -> {"data_id", "loss" (mean of the batch losses), "predictions", "labels"}"""
        m, lib = self.model, _lib.lib()
        class_weight = self._class_weight(loss_fn, class_weight)
        m.eval()
        ids_all, preds, labels, losses, accs = [], [], [], [], []
        with torch.no_grad():
            for dl in dataloader:
                out = m._engine_forward(dl["pixel_values"])
                onehot, cw = self._labels(dl["labels"], class_weight)
                loss = torch.empty(1, device=self.device)
                _lib.check(lib.mmhip_img_loss(m._handle, _lib.ptr(onehot), _lib.ptr(cw), _lib.ptr(loss), None, _lib.stream_ptr()), "img_loss")
                losses.append(loss)
                pred, target = out.argmax(dim=1), onehot.argmax(dim=1)
                accs.append((pred == target).float().mean().reshape(1) * 100)
                preds.append(pred)
                labels.append(target)
                if "data_id" in dl:
                    ids_all.append(dl["data_id"])
        eval_loss = float(torch.cat(losses).mean().item()) if losses else float("nan")
        eval_acc = float(torch.cat(accs).mean().item()) if accs else float("nan")
        print(f"test loss: {eval_loss:.4f} test acc: {eval_acc:.4f}\n")
        return {"data_id": torch.cat(ids_all).cpu().numpy() if ids_all else np.zeros(0, dtype=np.int64), "loss": eval_loss,
                "predictions": torch.cat(preds).cpu().numpy() if preds else np.zeros(0, dtype=np.int64),
                "labels": torch.cat(labels).cpu().numpy() if labels else np.zeros(0, dtype=np.int64)}
