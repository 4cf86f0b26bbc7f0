"""Drop-in for the reference's text-only models and trainer (models/text_only.py), backed by libmmhip.so.

  BERT / BERNICE   same constructors, forward signatures and state_dict keys as reference models/text_only.py:27-53 (bert_model.*, linear.*);
                   forward + backward run the text tower of the HIP engine under its fused CLS classifier head (include/mmhip.h: mmhip_txt_*).
  TextModel        same role as reference models/text_only.py:68-268 (load_data, train, eval, the return dictionaries), with a fused step:
                   forward + loss + backward + AdamW on flat buffers in one native call.

The reference classifies last_hidden[:, 0, :]; the encoder's pooler is computed there and never consumed.  Its parameters are kept (checkpoint
keys), never computed here, receive no gradient and no optimizer step -- what torch does with `grad is None`.
There is no CPU / eager fallback: without the built library (or without a GPU) construction raises.
"""
import logging
import math
import os

import numpy as np
import torch

from . import _lib
from . import dist as mmdist
from .config import MODEL_DIR_DICT, TEXT_ARCH, metric_names
from .engine_module import FlatTrainer, WordTableEngineModule, _read_hf_dir, merge_ranges
from .utils import agg_metrics_val

logger = logging.getLogger(__name__)


def default_txt_arch(arch_name):
    a = dict(hidden=768, heads=12, inter=3072, layers=12, p_hidden=0.1, p_attn=0.1)
    a.update(TEXT_ARCH[arch_name])
    return a


class _TxtFunction(torch.autograd.Function):
    """autograd edge around the engine so that the reference's loss.backward() (text_only.py:163) works on the returned logits"""

    @staticmethod
    def forward(ctx, model, ids, mask, type_ids, *params):
        out = model._engine_forward(ids, mask, type_ids)
        ctx.model, ctx.token = model, model._fwd_token
        return out

    @staticmethod
    def backward(ctx, d_logits):
        model = ctx.model
        if ctx.token != model._fwd_token:
            raise RuntimeError("text-only model: backward() after another forward(); the engine keeps one set of activations")
        return (None,) * 4 + tuple(model._engine_backward_autograd(d_logits))


class _TextOnly(WordTableEngineModule):
    """shared body of BERT and BERNICE.  Keyword-only extras are additive, as in MM_Model: `arch` overrides (layer count, vocab ... for tests),
    `arch_name` (the TEXT_ARCH preset when model_dir holds no checkpoint), `dtype` ('bf16' | 'f16' | 'bf16x3'), `max_posts` / `max_text_len`
    (capacity), `device`, `seed`, `backward_products` (bf16x3 only)."""

    _default_arch_name = "bernice"
    # a text-only handle is an mmhip_handle: the stage ranges of the late-fusion family are read through its entry points (include/mmhip.h)
    _ABI = dict(create="mmhip_txt_create", destroy="mmhip_txt_destroy", param_count="mmhip_txt_param_count", param_info_at="mmhip_txt_param_info_at",
                workspace_bytes="mmhip_txt_workspace_bytes", num_stages="mmhip_num_backward_stages", stage_grad_range="mmhip_stage_grad_range")
    _embeddings = ("bert_model", "embeddings")

    def __init__(self, model_dir, num_labels, dropout=0.1, *, arch=None, arch_name=None, dtype="bf16", max_posts=64, max_text_len=128,
                 device=None, seed=0, backward_products=None):
        super().__init__()
        if not torch.cuda.is_available():
            raise _lib.MMHipError("the text-only model needs an MI355X (gfx950) GPU: the HIP path has no CPU fallback")
        self.num_labels = int(num_labels)
        self.device_ = torch.device(device if device is not None else f"cuda:{int(os.environ.get('LOCAL_RANK', 0))}")
        a = default_txt_arch(arch_name or self._default_arch_name)
        cfg, sd = _read_hf_dir(model_dir or "")
        if cfg:
            a.update(vocab=cfg["vocab_size"], max_pos=cfg["max_position_embeddings"], type_vocab=cfg.get("type_vocab_size", 1),
                     layers=cfg["num_hidden_layers"], ln_eps_txt=cfg.get("layer_norm_eps", 1e-12), pad_id=cfg.get("pad_token_id", a["pad_id"]),
                     p_hidden=cfg.get("hidden_dropout_prob", 0.1), p_attn=cfg.get("attention_probs_dropout_prob", 0.1),
                     txt_kind="bert" if cfg.get("model_type", "") == "bert" else "xlmr")
        a.update(arch or {})
        self.arch, self.dtype_name = a, dtype
        if backward_products is not None and (dtype != "bf16x3" or int(backward_products) not in (1, 2, 3)):
            raise ValueError("backward_products is 1, 2 or 3 and belongs to dtype='bf16x3'")
        self.backward_products = None if backward_products is None else int(backward_products)
        self._cfg_kw = dict(hidden=a["hidden"], heads=a["heads"], inter=a["inter"], layers=a["layers"], vocab=a["vocab"], max_pos=a["max_pos"],
                            type_vocab=a["type_vocab"], txt_kind=_lib.TXT_XLMR if a["txt_kind"] == "xlmr" else _lib.TXT_BERT, pad_id=a["pad_id"],
                            ln_eps=a["ln_eps_txt"], num_labels=self.num_labels, p_hidden=a["p_hidden"], p_attn=a["p_attn"], p_head=float(dropout),
                            dtype={"bf16": _lib.BF16, "f16": _lib.F16, "bf16x3": _lib.BF16X3}[dtype])
        self._init_engine(int(seed) if seed is not None else int(torch.initial_seed()))
        self._create_engine(max_posts, max_text_len)
        self._init_weights()
        if sd is not None:
            self._load_tower(sd)
        self._refresh_weights()

    # ------------------------------------------------------------------ engine / buffers
    def _config(self, max_posts, max_text_len):
        return _lib.TxtConfig(max_posts=int(max_posts), max_text_len=int(max_text_len), loss_scale=float(getattr(self, "_loss_scale", 0.0)), **self._cfg_kw)

    def _allocate_flats(self, h):
        n = _lib.lib().mmhip_txt_numel(h)
        self._flat_train = torch.zeros(n, dtype=torch.float32, device=self.device_)
        self._flat_grad = torch.zeros(n, dtype=torch.float32, device=self.device_)
        return {1: self._flat_train}

    def _bind(self, h):
        _lib.check(_lib.lib().mmhip_txt_bind(h, _lib.ptr(self._flat_train), _lib.ptr(self._flat_grad), _lib.ptr(self._ws), self._ws.numel()), "txt_bind")

    def _init_weights(self):
        """HF initializer_range 0.02 for the encoder, nn.Linear defaults for the classifier (reference: from_pretrained + nn.Linear)"""
        g = torch.Generator(device=self.device_).manual_seed(self._seed_base)
        with torch.no_grad():
            for inf in self._infos:
                n, p = inf["name"], inf["param"]
                if n.startswith("bert_model."):
                    if "LayerNorm.weight" in n:
                        p.fill_(1.0)
                    elif n.endswith(".bias"):
                        p.zero_()
                    else:
                        p.normal_(0.0, 0.02, generator=g)
                else:
                    bound = 1.0 / math.sqrt(self.arch["hidden"])
                    p.uniform_(-bound, bound, generator=g)
            self._modules["bert_model"]._modules["embeddings"]._modules["word_embeddings"].weight[self.arch["pad_id"]].zero_()

    def _load_tower(self, sd):
        own = {inf["name"]: inf["param"] for inf in self._infos}
        with torch.no_grad():
            for k, v in sd.items():
                for strip in ("bert.", "roberta.", ""):
                    name = "bert_model." + k[len(strip):]
                    if k.startswith(strip) and name in own and tuple(own[name].shape) == tuple(v.shape):
                        own[name].copy_(v.to(own[name].device, torch.float32))
                        break

    def _refresh_weights(self):
        _lib.check(_lib.lib().mmhip_txt_refresh_weights(self._handle, _lib.stream_ptr()), "txt_refresh_weights")
        self._weights_version = self._flat_train._version

    def _ensure(self, B, T):
        cap_b, cap_t = self._capacity
        if B > cap_b or T > cap_t:
            self._create_engine(max(B, cap_b), max(T, cap_t))
            self._refresh_weights()
        elif self._weights_version != self._flat_train._version:
            self._refresh_weights()        # parameters were modified in place (optimizer.step / load_state_dict)

    def _inputs(self, ids, mask, type_ids):
        dev = self.device_
        ids = ids.to(dev, torch.int64).contiguous()
        mask = mask.to(dev, torch.int64).contiguous()
        if ids.dim() != 2 or mask.shape != ids.shape:
            raise ValueError(f"text-only forward: ids {tuple(ids.shape)}, mask {tuple(mask.shape)}")
        if type_ids is not None:
            type_ids = type_ids.to(dev, torch.int64).contiguous()
            if type_ids.shape != ids.shape:
                raise ValueError(f"token_type_ids {tuple(type_ids.shape)} for ids {tuple(ids.shape)}")
        return ids, mask, type_ids

    def _engine_forward(self, ids, mask, type_ids=None, seed=None):
        ids, mask, type_ids = self._inputs(ids, mask, type_ids)
        B, T = ids.shape
        self._ensure(B, T)
        seed = self._next_seed() if seed is None else seed
        logits = torch.empty(B, self.num_labels, device=self.device_)
        _lib.check(_lib.lib().mmhip_txt_forward(self._handle, _lib.ptr(ids), _lib.ptr(mask), _lib.ptr(type_ids), B, T, int(self.training), seed,
                                                _lib.ptr(logits), _lib.stream_ptr()), "txt_forward")
        self._fwd_token += 1
        self._last = dict(B=B, T=T, seed=seed, ids=ids)
        return logits

    def trainable_infos(self):
        """parameters that receive a gradient: everything but the never-consumed pooler (MMHIP_G_NEVER)"""
        return [i for i in self._infos if i["group"] != _lib.G_NEVER]

    def active_ranges(self):
        """merged [begin, end) element ranges of the flat buffer that AdamW steps"""
        return merge_ranges((i["offset"], i["numel"]) for i in self.trainable_infos())

    def _engine_backward(self, d_logits=None):
        """gradient of the last forward into the flat gradient buffer (cleared first); d_logits None: the one mmhip_txt_loss left in the handle"""
        self._zero_grad_state()
        if d_logits is not None:
            d_logits = d_logits.to(self.device_, torch.float32).contiguous()
        _lib.check(_lib.lib().mmhip_txt_backward(self._handle, _lib.ptr(d_logits), _lib.stream_ptr()), "txt_backward")
        self._grad_dirty = True

    def _engine_backward_autograd(self, d_logits):
        self._engine_backward(d_logits)
        return [None if inf["group"] == _lib.G_NEVER else self._flat_grad[inf["offset"]: inf["offset"] + inf["numel"]].view(inf["shape"]).clone()
                for inf in self._infos]

    def _forward(self, ids, mask, type_ids):
        if torch.is_grad_enabled() and any(i["param"].requires_grad for i in self._infos):
            return _TxtFunction.apply(self, ids, mask, type_ids, *[i["param"] for i in self._infos])
        return self._engine_forward(ids, mask, type_ids)


class BERNICE(_TextOnly):
    """reference models/text_only.py:41-53: forward(ids, mask) -> linear(dropout(last_hidden[:, 0, :]))"""
    _default_arch_name = "bernice"

    def forward(self, ids, mask):
        return self._forward(ids, mask, None)


class BERT(_TextOnly):
    """reference models/text_only.py:27-39: forward(ids, mask, token_type_ids).  A one-row type table (RoBERTa-shaped checkpoints such as
    bertweet) takes row 0 for every token, as HF does with all-zero type ids."""
    _default_arch_name = "bert"

    def forward(self, ids, mask, token_type_ids):
        return self._forward(ids, mask, token_type_ids)


# =====================================================================================================================
class TextModel(FlatTrainer):
    """reference models/text_only.py:68-268.  `train()` / `eval()` keep the reference's semantics and return dictionaries; the step is fused."""

    def __init__(self, config, model_name, freeze=False, **model_kw):
        if freeze:
            raise NotImplementedError("freeze=True: the reference's command line never passes it (models/run_txt.py:51); the HIP step trains the encoder")
        if getattr(config, "use_loss_correction", False):
            raise NotImplementedError("--use_loss_correction is not part of this build (as in the other trainers here)")
        if model_name == "roberta":
            raise NotImplementedError("roberta: the reference itself fails here -- models/text_only.py:90 assigns the model to a local variable, "
                                      "so TextModel has no .model -- and its RoBERTa class classifies the un-dropped pooled output (:63-65)")
        if model_name not in TEXT_ARCH:
            raise ValueError(f"text model {model_name!r}: the text-only path supports {sorted(set(TEXT_ARCH) - {'roberta'})}")
        if mmdist.world_size() > 1:
            raise NotImplementedError("the text-only trainer is single-process: data-parallel training of this path is not implemented "
                                      f"(world size {mmdist.world_size()}); launch one process")
        self.batch_size, self.num_labels = config.batch_size, config.num_labels
        self.model_name, self.model_dir = model_name, MODEL_DIR_DICT[model_name]
        self.max_length, self.dropout = config.max_length, config.dropout
        self.use_loss_correction = False
        self.tokenizer = None                       # created by load_data (real data keys only)
        model_kw.setdefault("max_posts", config.batch_size)
        model_kw.setdefault("max_text_len", config.max_length)
        model_kw.setdefault("arch_name", model_name)
        cls = BERNICE if model_name == "bernice" else BERT          # bert, and the reference's `else` branch (bertweet)
        self.model = cls(self.model_dir, self.num_labels, dropout=self.dropout, **model_kw)
        self.with_types = model_name not in {"roberta", "bernice"}
        self.device = self.model.device_
        self._opt = None

    # ---- data
    def load_data(self, data, testing=False, eval_txt_test=False, task_name=None):
        """reference :105-121 -> (train_loader, val_loader, test_loader, class_weights, txt_te_loader)"""
        from transformers import AutoTokenizer
        from .datasets import TxtOnly_Dataset, prepare_data
        if eval_txt_test:
            raise NotImplementedError("--eval_txt_test needs the reference's separate text-only test key (models/utils.py prepare_text_data): not part of this build")
        if self.tokenizer is None:
            kw = dict(model_max_length=self.max_length) if self.model_name == "bernice" else {}
            self.tokenizer = AutoTokenizer.from_pretrained(self.model_dir, **kw)
        tr, ytr, va, yva, te, yte, w = prepare_data(data, self.num_labels, testing=testing)
        mk = lambda df, y: TxtOnly_Dataset(self.model_name, df.tweet_id.values, df.text.values, y, self.tokenizer, self.max_length, task_name)
        dl = lambda ds, sh: torch.utils.data.DataLoader(ds, batch_size=self.batch_size, shuffle=sh)
        return dl(mk(tr, ytr), True), dl(mk(va, yva), False), dl(mk(te, yte), False), w, None

    def _batch(self, dl):
        """a loader item on the device, right padding beyond the batch's longest post trimmed (image_processing.DevicePrefetcher.trim)"""
        from .image_processing import DevicePrefetcher
        b = {"input_ids": dl["ids"], "attention_mask": dl["mask"]}
        if self.with_types and "token_type_ids" in dl:
            b["token_type_ids"] = dl["token_type_ids"]
        b = DevicePrefetcher.trim(b)
        to = lambda t: t.to(self.device, non_blocking=True)
        return to(b["input_ids"]), to(b["attention_mask"]), (to(b["token_type_ids"]) if "token_type_ids" in b else None)

    # ---- one fused training step on device tensors -> (loss[1] device tensor, n_correct[1] device tensor)
    def train_step(self, ids, mask, token_type_ids, onehot, class_weight, lr, weight_decay, step, seed=None):
        m = self.model
        if not m.training:
            m.train()
        m._clean_grad()
        ids, mask, token_type_ids = m._inputs(ids, mask, token_type_ids if self.with_types else None)
        B, T = ids.shape
        m._ensure(B, T)
        em, ev = self._moments()
        onehot = onehot.to(self.device, torch.int64).contiguous()
        cw = None if class_weight is None else class_weight.to(self.device, torch.float32).contiguous()
        loss = torch.empty(1, device=self.device)
        ncorr = torch.empty(1, dtype=torch.int32, device=self.device)
        seed = m._next_seed() if seed is None else seed
        m._last = dict(B=B, T=T, seed=seed, ids=ids)
        _lib.check(_lib.lib().mmhip_txt_train_step(m._handle, _lib.ptr(ids), _lib.ptr(mask), _lib.ptr(token_type_ids), _lib.ptr(onehot), _lib.ptr(cw),
                                                   B, T, seed, _lib.ptr(em), _lib.ptr(ev), lr, 0.9, 0.999, 1e-8, weight_decay, step,
                                                   _lib.ptr(loss), _lib.ptr(ncorr), _lib.stream_ptr()), "txt_train_step")
        m._fwd_token += 1
        m._weights_version = m._flat_train._version          # the refresh inside the call keeps the 16-bit copies current
        return loss, ncorr

    # ---- the same step as separate calls (forward, loss, backward, AdamW): what the fused call is checked against
    def staged_step(self, ids, mask, token_type_ids, onehot, class_weight, lr, weight_decay, step, seed=None):
        m, lib = self.model, _lib.lib()
        if not m.training:
            m.train()
        m._clean_grad()
        m._engine_forward(ids, mask, token_type_ids if self.with_types else None, seed=seed)
        onehot = onehot.to(self.device, torch.int64).contiguous()
        cw = None if class_weight is None else class_weight.to(self.device, torch.float32).contiguous()
        loss = torch.empty(1, device=self.device)
        ncorr = torch.empty(1, dtype=torch.int32, device=self.device)
        _lib.check(lib.mmhip_txt_loss(m._handle, _lib.ptr(onehot), _lib.ptr(cw), _lib.ptr(loss), _lib.ptr(ncorr), _lib.stream_ptr()), "txt_loss")
        m._engine_backward(None)
        self._adamw_ranges(m.active_ranges(), lr, weight_decay, step, 1.0)
        m._grad_dirty = False
        m._refresh_weights()
        return loss, ncorr

    def _clamped_message(self, n):
        return f"index out of range in self: {n} token id(s) outside the embedding tables reached the text tower"

    def check_overflow(self):
        n = int(self.model._nonfinite[0].item()) - getattr(self, "_nf_seen", 0)
        if n > 0:
            self._nf_seen = getattr(self, "_nf_seen", 0) + n
            if self.model.dtype_name != "f16":
                raise FloatingPointError(f"non-finite gradients met {n} times ({self.model.dtype_name}): the run has diverged")
            logger.warning("f16 gradient overflow: %d step(s) were skipped on the device", n)
        return max(n, 0)

    def train(self, dataloader, val_dataloader, epochs, loss_fn=None, lr=1e-5, weight_decay=0.00025, te_dataloader=None, model_path=None,
              val_filename=None, te_filename=None, class_weight=None, log_every=50):
        """reference :124-202.  `loss_fn` is accepted for signature parity: the class weights it carries (nn.CrossEntropyLoss(weight=w),
        run_txt.py:54) are what the fused step uses."""
        import pandas as pd
        class_weight = self._class_weight(loss_fn, class_weight)
        res_val, res_te, step = [], [], 0
        for epoch in range(epochs):
            print(epoch)
            for it, dl in enumerate(dataloader):
                ids, mask, tt = self._batch(dl)
                step += 1
                loss, ncorr = self.train_step(ids, mask, tt, dl["target"], class_weight, lr, weight_decay, step)
                if log_every and it % log_every == 0:          # the reference syncs and prints every step (:166-171)
                    self.check_overflow()
                    n = ids.shape[0]
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
        """reference :204-268 -> {"data_id", "loss" (mean of the batch losses), "predictions", "labels"}"""
        m, lib = self.model, _lib.lib()
        class_weight = self._class_weight(loss_fn, class_weight)
        cw = None if class_weight is None else class_weight.to(self.device, torch.float32).contiguous()
        m.eval()
        ids_all, preds, labels, losses, accs = [], [], [], [], []
        with torch.no_grad():
            for dl in dataloader:
                ids, mask, tt = self._batch(dl)
                out = m._engine_forward(ids, mask, tt)
                onehot = dl["target"].to(self.device, torch.int64).contiguous()
                loss = torch.empty(1, device=self.device)
                _lib.check(lib.mmhip_txt_loss(m._handle, _lib.ptr(onehot), _lib.ptr(cw), _lib.ptr(loss), None, _lib.stream_ptr()), "txt_loss")
                losses.append(loss)
                pred, target = out.argmax(dim=1), onehot.argmax(dim=1)
                accs.append((pred == target).float().mean().reshape(1) * 100)
                preds.append(pred)
                labels.append(target)
                if "data_id" in dl:
                    ids_all.append(dl["data_id"])
        eval_loss = float(torch.cat(losses).mean().item()) if losses else float("nan")
        eval_acc = float(torch.cat(accs).mean().item()) if accs else float("nan")
        print(f"loss: {eval_loss:.4f} acc: {eval_acc:.4f}\n")
        self.check_indices()
        return {"data_id": torch.cat(ids_all).cpu().numpy() if ids_all else np.zeros(0, dtype=np.int64), "loss": eval_loss,
                "predictions": torch.cat(preds).cpu().numpy() if preds else np.zeros(0, dtype=np.int64),
                "labels": torch.cat(labels).cpu().numpy() if labels else np.zeros(0, dtype=np.int64)}
