"""One tower under a fused classifier head: what the text-only (text_only.py, mmhip_txt_*) and the image-only (image_only.py, mmhip_img_*) front
ends share.  Both families have one trainable flat buffer and its gradient, the same entry points up to the family tag in their names, the same
autograd edge and the same trainer: a fused step, the staged step it is checked against, the reference's epoch loop and evaluation.

A family keeps what differs: its constructor's signature and refusals, input validation (`_inputs`), the argument lists of the two native calls
whose signatures differ (`_forward_args`, `_step_args`), its initialisation and checkpoint keys, how a loader item becomes engine inputs and a
one-hot target (`_item`), `load_data`, and `forward()`.
"""
import logging
import os

import numpy as np
import torch

from . import _lib
from .config import metric_names
from .engine_module import FlatTrainer, _read_hf_dir, merge_ranges
from .utils import agg_metrics_val

logger = logging.getLogger(__name__)


def tower_abi(family):
    """EngineModule._ABI of a one-tower family ('txt' | 'img').  Such a handle is an mmhip_handle: its stage ranges are read through the
    late-fusion family's two entry points (include/mmhip.h)"""
    own = {k: f"mmhip_{family}_{k}" for k in ("create", "destroy", "param_count", "param_info_at", "workspace_bytes")}
    return dict(own, num_stages="mmhip_num_backward_stages", stage_grad_range="mmhip_stage_grad_range")


class _TowerFunction(torch.autograd.Function):
    """autograd edge around the engine so that the reference's loss.backward() works on the returned logits"""

    @staticmethod
    def forward(ctx, model, n_inputs, *inputs_and_params):
        out = model._engine_forward(*inputs_and_params[:n_inputs])
        ctx.model, ctx.token, ctx.n_inputs = model, model._fwd_token, n_inputs
        return out

    @staticmethod
    def backward(ctx, d_logits):
        model = ctx.model
        if ctx.token != model._fwd_token:
            raise RuntimeError(f"{model._what} model: backward() after another forward(); the engine keeps one set of activations")
        return (None,) * (2 + ctx.n_inputs) + tuple(model._engine_backward_autograd(d_logits))


class OneTowerModule:
    """mixed into a GuardedEngineModule.  The family sets the four names below and provides `_arch_from_hf(cfg, arch)` (config.json -> arch
    entries), `_cfg_keywords(arch)` (arch -> the config struct's own fields), `_init_weights()`, `_load_checkpoint(state_dict)`,
    `_inputs(*raw)` (-> the validated device tensors, the batch first) and the two argument lists."""

    _family = ""              # 'txt' | 'img': mmhip_<family>_* are the family's entry points
    _what = ""                # 'text-only' | 'image-only', as the messages name the model
    _Config = None            # the family's config struct
    _capacity_names = ()      # its capacity fields: the leading dimensions of the first input

    def _build(self, model_dir, num_labels, default_arch, arch, dtype, capacity, device, seed, backward_products, **cfg_kw):
        """the constructor after nn.Module's: arch defaults <- config.json of `model_dir` <- `arch` overrides, the engine, the initial weights,
        the checkpoint of `model_dir`"""
        if not torch.cuda.is_available():
            raise _lib.MMHipError(f"the {self._what} model needs an MI355X (gfx950) GPU: the HIP path has no CPU fallback")
        self.num_labels = int(num_labels)
        self.device_ = torch.device(device if device is not None else f"cuda:{int(os.environ.get('LOCAL_RANK', 0))}")
        a = default_arch
        cfg, sd = _read_hf_dir(model_dir or "")
        if cfg:
            a.update(self._arch_from_hf(cfg, a))
        a.update(arch or {})
        self.arch, self.dtype_name = a, dtype
        if backward_products is not None and (dtype != "bf16x3" or int(backward_products) not in (1, 2, 3)):
            raise ValueError("backward_products is 1, 2 or 3 and belongs to dtype='bf16x3'")
        self.backward_products = None if backward_products is None else int(backward_products)
        self._cfg_kw = dict(self._cfg_keywords(a), hidden=a["hidden"], heads=a["heads"], inter=a["inter"], layers=a["layers"], num_labels=self.num_labels,
                            p_hidden=a["p_hidden"], p_attn=a["p_attn"], dtype={"bf16": _lib.BF16, "f16": _lib.F16, "bf16x3": _lib.BF16X3}[dtype], **cfg_kw)
        self._init_engine(int(seed) if seed is not None else int(torch.initial_seed()))
        self._create_engine(*capacity)
        self._init_weights()
        if sd is not None:
            self._load_checkpoint(sd)
        self._refresh_weights()

    # ------------------------------------------------------------------ engine / buffers
    def _native(self, name, *args):
        _lib.check(getattr(_lib.lib(), f"mmhip_{self._family}_{name}")(self._handle, *args), f"{self._family}_{name}")

    def _config(self, *capacity):
        return self._Config(loss_scale=float(self._loss_scale), **dict(zip(self._capacity_names, map(int, capacity))), **self._cfg_kw)

    def _allocate_flats(self, h):
        n = getattr(_lib.lib(), f"mmhip_{self._family}_numel")(h)
        self._flat_train = torch.zeros(n, dtype=torch.float32, device=self.device_)
        self._flat_grad = torch.zeros(n, dtype=torch.float32, device=self.device_)
        return {1: self._flat_train}

    def _bind(self, h):
        self._native("bind", _lib.ptr(self._flat_train), _lib.ptr(self._flat_grad), _lib.ptr(self._ws), self._ws.numel())

    def _refresh_weights(self):
        self._native("refresh_weights", _lib.stream_ptr())
        self._weights_version = self._flat_train._version

    def _ensure(self, *need):
        if any(n > c for n, c in zip(need, self._capacity)):
            self._create_engine(*(max(n, c) for n, c in zip(need, self._capacity)))
            self._refresh_weights()
        elif self._weights_version != self._flat_train._version:
            self._refresh_weights()        # parameters were modified in place (optimizer.step / load_state_dict)

    def _checked(self, *raw):
        """-> the validated inputs, with an engine that holds them and current 16-bit weights"""
        inputs = self._inputs(*raw)
        self._ensure(*inputs[0].shape[: len(self._capacity)])
        return inputs

    def _engine_forward(self, *raw, seed=None):
        inputs = self._checked(*raw)
        logits = torch.empty(inputs[0].shape[0], self.num_labels, device=self.device_)
        self._native("forward", *self._forward_args(seed, *inputs), _lib.ptr(logits), _lib.stream_ptr())
        self._fwd_token += 1
        return logits

    def trainable_infos(self):
        """parameters that receive a gradient: everything but what the model never consumes (MMHIP_G_NEVER: the text encoder's pooler)"""
        return [i for i in self._infos if i["group"] != _lib.G_NEVER]

    def active_ranges(self):
        """merged [begin, end) element ranges of the flat buffer that AdamW steps"""
        return merge_ranges((i["offset"], i["numel"]) for i in self.trainable_infos())

    def _engine_backward(self, d_logits=None):
        """gradient of the last forward into the flat gradient buffer (cleared first); d_logits None: the one the loss call left in the handle"""
        self._zero_grad_state()
        if d_logits is not None:
            d_logits = d_logits.to(self.device_, torch.float32).contiguous()
        self._native("backward", _lib.ptr(d_logits), _lib.stream_ptr())
        self._grad_dirty = True

    def _engine_backward_autograd(self, d_logits):
        self._engine_backward(d_logits)
        return [None if inf["group"] == _lib.G_NEVER else self._flat_grad[inf["offset"]: inf["offset"] + inf["numel"]].view(inf["shape"]).clone()
                for inf in self._infos]

    def _logits(self, *inputs):
        if torch.is_grad_enabled() and any(i["param"].requires_grad for i in self._infos):
            return _TowerFunction.apply(self, len(inputs), *inputs, *[i["param"] for i in self._infos])
        return self._engine_forward(*inputs)


# =====================================================================================================================
class OneTowerTrainer(FlatTrainer):
    """the reference's trainers over one tower (models/text_only.py:68-268, models/image_only.py:122-317): `train()` / `eval()` keep their
    semantics and return dictionaries; the step is fused.  A step's arguments are the engine inputs, then `onehot, class_weight, lr,
    weight_decay, step`."""

    _opt = None               # (m, v) of AdamW, made by the first step
    _overflow_note = ""       # what the device did with an f16 overflow, for the warning
    _eval_line = ""           # format of eval()'s print: loss, accuracy

    def _item(self, dl):
        """a loader item -> (engine inputs, one-hot target)"""
        raise NotImplementedError

    def _engine_inputs(self, *inputs):
        """of a step's inputs, what the model takes"""
        return inputs

    def _dev(self, t, dtype):
        return None if t is None else t.to(self.device, dtype).contiguous()

    def _begin_step(self, onehot, class_weight):
        m = self.model
        if not m.training:
            m.train()
        m._clean_grad()
        return (self._dev(onehot, torch.int64), self._dev(class_weight, torch.float32), torch.empty(1, device=self.device),
                torch.empty(1, dtype=torch.int32, device=self.device))

    # ---- one fused training step on device tensors -> (loss[1] device tensor, n_correct[1] device tensor)
    def train_step(self, *args, seed=None):
        *inputs, onehot, class_weight, lr, weight_decay, step = args
        m = self.model
        onehot, cw, loss, ncorr = self._begin_step(onehot, class_weight)
        inputs = m._checked(*self._engine_inputs(*inputs))
        em, ev = self._moments()
        m._native("train_step", *m._step_args(seed, onehot, cw, *inputs), _lib.ptr(em), _lib.ptr(ev), lr, 0.9, 0.999, 1e-8, weight_decay, step,
                  _lib.ptr(loss), _lib.ptr(ncorr), _lib.stream_ptr())
        m._fwd_token += 1
        m._weights_version = m._flat_train._version          # the refresh inside the call keeps the 16-bit copies current
        return loss, ncorr

    # ---- the same step as separate calls (forward, loss, backward, AdamW): what the fused call is checked against
    def staged_step(self, *args, seed=None):
        *inputs, onehot, class_weight, lr, weight_decay, step = args
        m = self.model
        onehot, cw, loss, ncorr = self._begin_step(onehot, class_weight)
        m._engine_forward(*self._engine_inputs(*inputs), seed=seed)
        m._native("loss", _lib.ptr(onehot), _lib.ptr(cw), _lib.ptr(loss), _lib.ptr(ncorr), _lib.stream_ptr())
        m._engine_backward(None)
        self._grad_clip_norm(m.active_ranges(), 1.0)
        self._adamw_ranges(m.active_ranges(), lr, weight_decay, step, 1.0)
        m._grad_dirty = False
        m._refresh_weights()
        return loss, ncorr

    def check_overflow(self):
        n = int(self.model._nonfinite[0].item()) - getattr(self, "_nf_seen", 0)
        if n > 0:
            self._nf_seen = getattr(self, "_nf_seen", 0) + n
            if self.model.dtype_name != "f16":
                raise FloatingPointError(f"non-finite gradients met {n} times ({self.model.dtype_name}): the run has diverged")
            logger.warning("f16 gradient overflow: %d " + self._overflow_note + " on the device", n)
        return max(n, 0)

    def train(self, dataloader, val_dataloader, epochs, loss_fn=None, lr=1e-5, weight_decay=0.00025, te_dataloader=None, model_path=None,
              val_filename=None, te_filename=None, class_weight=None, log_every=50):
        """reference text_only.py:124-202, image_only.py:179-258.  `loss_fn` is accepted for signature parity: the class weights it carries
        (nn.CrossEntropyLoss(weight=w), run_txt.py:54, run_img.py:56) are what the fused step uses."""
        import pandas as pd
        class_weight = self._class_weight(loss_fn, class_weight)
        res_val, res_te, step = [], [], 0
        for epoch in range(epochs):
            print(epoch)
            for it, dl in enumerate(dataloader):
                inputs, target = self._item(dl)
                step += 1
                loss, ncorr = self.train_step(*inputs, target, class_weight, lr, weight_decay, step)
                if log_every and it % log_every == 0:          # the reference syncs and prints every step
                    self.check_overflow()
                    n = target.shape[0]
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
            self._log_grad_clip()
        if model_path is not None:
            self.save_model(model_path)
            logger.info("%s saved", model_path)

    def eval(self, dataloader, loss_fn=None, class_weight=None):
        """reference text_only.py:204-268, image_only.py:260-317 -> {"data_id", "loss" (mean of the batch losses), "predictions", "labels"}"""
        m = self.model
        cw = self._dev(self._class_weight(loss_fn, class_weight), torch.float32)
        m.eval()
        ids_all, preds, labels, losses, accs = [], [], [], [], []
        with torch.no_grad():
            for dl in dataloader:
                inputs, onehot = self._item(dl)
                out = m._engine_forward(*inputs)
                onehot = self._dev(onehot, torch.int64)
                loss = torch.empty(1, device=self.device)
                m._native("loss", _lib.ptr(onehot), _lib.ptr(cw), _lib.ptr(loss), None, _lib.stream_ptr())
                losses.append(loss)
                pred, target = out.argmax(dim=1), onehot.argmax(dim=1)
                accs.append((pred == target).float().mean().reshape(1) * 100)
                preds.append(pred)
                labels.append(target)
                if "data_id" in dl:
                    ids_all.append(dl["data_id"])
        eval_loss = float(torch.cat(losses).mean().item()) if losses else float("nan")
        eval_acc = float(torch.cat(accs).mean().item()) if accs else float("nan")
        print(self._eval_line.format(eval_loss, eval_acc))
        if m._word_info is not None:          # ids that had to be clamped into the word table raise here, as they do in the reference's embedding
            self.check_indices()
        cat = lambda parts: torch.cat(parts).cpu().numpy() if parts else np.zeros(0, dtype=np.int64)
        return {"data_id": cat(ids_all), "loss": eval_loss, "predictions": cat(preds), "labels": cat(labels)}
