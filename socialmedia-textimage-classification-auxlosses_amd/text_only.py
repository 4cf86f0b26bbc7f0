"""Drop-in for the reference's text-only models and trainer (models/text_only.py), backed by libmmhip.so.

  BERT / BERNICE   same constructors, forward signatures and state_dict keys as reference models/text_only.py:27-53 (bert_model.*, linear.*);
                   forward + backward run the text tower of the HIP engine under its fused CLS classifier head (include/mmhip.h: mmhip_txt_*).
  TextModel        same role as reference models/text_only.py:68-268 (load_data, train, eval, the return dictionaries), with a fused step:
                   forward + loss + backward + AdamW on flat buffers in one native call.

The reference classifies last_hidden[:, 0, :]; the encoder's pooler is computed there and never consumed.  Its parameters are kept (checkpoint
keys), never computed here, receive no gradient and no optimizer step -- what torch does with `grad is None`.
What this family shares with the image-only one -- the engine plumbing, the autograd edge, the trainer's steps, epoch loop and evaluation --
is one_tower.py.  There is no CPU / eager fallback: without the built library (or without a GPU) construction raises.
"""
import math

import torch

from . import _lib
from . import dist as mmdist
from .config import MODEL_DIR_DICT, TEXT_ARCH
from .engine_module import WordTableEngineModule
from .one_tower import OneTowerModule, OneTowerTrainer, tower_abi


def default_txt_arch(arch_name):
    a = dict(hidden=768, heads=12, inter=3072, layers=12, p_hidden=0.1, p_attn=0.1)
    a.update(TEXT_ARCH[arch_name])
    return a


class _TextOnly(OneTowerModule, WordTableEngineModule):
    """shared body of BERT and BERNICE.  Keyword-only extras are additive, as in MM_Model: `arch` overrides (layer count, vocab ... for tests),
    `arch_name` (the TEXT_ARCH preset when model_dir holds no checkpoint), `dtype` ('bf16' | 'f16' | 'bf16x3'), `max_posts` / `max_text_len`
    (capacity), `device`, `seed`, `backward_products` (bf16x3 only)."""

    _default_arch_name = "bernice"
    _family, _what, _ABI = "txt", "text-only", tower_abi("txt")
    _Config, _capacity_names = _lib.TxtConfig, ("max_posts", "max_text_len")
    _embeddings = ("bert_model", "embeddings")

    def __init__(self, model_dir, num_labels, dropout=0.1, *, arch=None, arch_name=None, dtype="bf16", max_posts=64, max_text_len=128,
                 device=None, seed=0, backward_products=None):
        super().__init__()
        self._build(model_dir, num_labels, default_txt_arch(arch_name or self._default_arch_name), arch, dtype, (max_posts, max_text_len), device,
                    seed, backward_products, p_head=float(dropout))

    @staticmethod
    def _arch_from_hf(cfg, a):
        return dict(vocab=cfg["vocab_size"], max_pos=cfg["max_position_embeddings"], type_vocab=cfg.get("type_vocab_size", 1),
                    layers=cfg["num_hidden_layers"], ln_eps_txt=cfg.get("layer_norm_eps", 1e-12), pad_id=cfg.get("pad_token_id", a["pad_id"]),
                    p_hidden=cfg.get("hidden_dropout_prob", 0.1), p_attn=cfg.get("attention_probs_dropout_prob", 0.1),
                    txt_kind="bert" if cfg.get("model_type", "") == "bert" else "xlmr")

    @staticmethod
    def _cfg_keywords(a):
        return dict(vocab=a["vocab"], max_pos=a["max_pos"], type_vocab=a["type_vocab"], pad_id=a["pad_id"], ln_eps=a["ln_eps_txt"],
                    txt_kind=_lib.TXT_XLMR if a["txt_kind"] == "xlmr" else _lib.TXT_BERT)

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

    def _load_checkpoint(self, sd):
        own = {inf["name"]: inf["param"] for inf in self._infos}
        with torch.no_grad():
            for k, v in sd.items():
                for strip in ("bert.", "roberta.", ""):
                    name = "bert_model." + k[len(strip):]
                    if k.startswith(strip) and name in own and tuple(own[name].shape) == tuple(v.shape):
                        own[name].copy_(v.to(own[name].device, torch.float32))
                        break

    def _inputs(self, ids, mask, type_ids=None):
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

    def _seeded(self, seed, ids, mask, type_ids):
        """one dropout seed per engine call unless the caller brings one; -> the arguments both native calls begin with, B, T, seed"""
        B, T = ids.shape
        seed = self._next_seed() if seed is None else seed
        self._last = dict(B=B, T=T, seed=seed, ids=ids)
        return [_lib.ptr(ids), _lib.ptr(mask), _lib.ptr(type_ids)], B, T, seed

    def _forward_args(self, seed, *inputs):
        ptrs, B, T, seed = self._seeded(seed, *inputs)
        return ptrs + [B, T, int(self.training), seed]

    def _step_args(self, seed, onehot, cw, *inputs):
        ptrs, B, T, seed = self._seeded(seed, *inputs)
        return ptrs + [_lib.ptr(onehot), _lib.ptr(cw), B, T, seed]


class BERNICE(_TextOnly):
    """reference models/text_only.py:41-53: forward(ids, mask) -> linear(dropout(last_hidden[:, 0, :]))"""
    _default_arch_name = "bernice"

    def forward(self, ids, mask):
        return self._logits(ids, mask, None)


class BERT(_TextOnly):
    """reference models/text_only.py:27-39: forward(ids, mask, token_type_ids).  A one-row type table (RoBERTa-shaped checkpoints such as
    bertweet) takes row 0 for every token, as HF does with all-zero type ids."""
    _default_arch_name = "bert"

    def forward(self, ids, mask, token_type_ids):
        return self._logits(ids, mask, token_type_ids)


# =====================================================================================================================
class TextModel(OneTowerTrainer):
    """reference models/text_only.py:68-268.  A step takes `ids, mask, token_type_ids, onehot, class_weight, lr, weight_decay, step`."""

    _overflow_note = "step(s) were skipped"
    _eval_line = "loss: {:.4f} acc: {:.4f}\n"

    def __init__(self, config, model_name, freeze=False, max_grad_norm=None, **model_kw):
        self._refuse_grad_clip_under_dp(max_grad_norm, mmdist.world_size())
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
        self.set_max_grad_norm(max_grad_norm)

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

    def _item(self, dl):
        return self._batch(dl), dl["target"]

    def _engine_inputs(self, ids, mask, token_type_ids):
        return ids, mask, token_type_ids if self.with_types else None

    def _clamped_message(self, n):
        return f"index out of range in self: {n} token id(s) outside the embedding tables reached the text tower"
