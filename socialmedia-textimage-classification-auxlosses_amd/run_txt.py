"""Command line of the text-only runs -- same flags, defaults, file names and CSV layouts as the reference's models/run_txt.py:19-104.
Additive flags: --synthetic / --n_synthetic (no dataset on disk), --dtype, --batch_size, --results_dir, --arch_layers, --max_grad_norm.  Single process.

    python -m smtc_amd.run_txt --model_name bernice --task 3 --testing
"""
import argparse
import logging
import os
import sys

import numpy as np
import pandas as pd
import torch

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import smtc_amd  # noqa: F401
    __package__ = "smtc_amd"

from . import dist as mmdist
from .config import Config, results_dir_txt
from .synthetic import synthetic_batch
from .utils import compute_metrics, balanced_class_weights

logging.basicConfig(format="%(asctime)s - %(message)s", datefmt="%Y-%m-%d %H:%M:%S", level=logging.INFO)
logger = logging.getLogger(__name__)


def build_parser():
    p = argparse.ArgumentParser(description="run text-only models")
    # reference flags, models/run_txt.py:20-31 (names, types, choices, defaults unchanged)
    p.add_argument("--model_name", type=str, choices=["bert", "bernice", "bertweet", "roberta"], help="model name")
    p.add_argument("--task", type=int, choices=[0, 1, 2, 3, 4, 5, 6], help="task to run")
    p.add_argument("--use_loss_correction", action="store_true", help="use Loss correction (only for binary cases)")
    p.add_argument("--epochs", type=int, default=2, help="number of epochs")
    p.add_argument("--weight_decay", type=float, default=0.00025, help="weight decay param")
    p.add_argument("--lr", type=float, default=1e-5, help="learning rate param")
    p.add_argument("--dropout", type=float, default=0.05, help="dropout param")
    p.add_argument("--seed", type=int, default=30, help="manual seed")
    p.add_argument("--testing", action="store_true", help="testing sample")
    p.add_argument("--eval_txt_test", action="store_true", help="eval txt test")
    p.add_argument("--save_model", action="store_true", help="save model")
    p.add_argument("--save_preds", action="store_true", help="eval test")
    # additive
    p.add_argument("--batch_size", type=int, default=None, help="batch size (default: the reference's per-task value)")
    p.add_argument("--synthetic", action="store_true", help="synthetic posts instead of the data key")
    p.add_argument("--n_synthetic", type=int, default=256, help="synthetic training posts")
    p.add_argument("--dtype", choices=["bf16", "f16", "bf16x3"], default="bf16", help="bf16x3 = strict-parity mode (fp32 activations, 3 bf16 MFMA products per Linear)")
    p.add_argument("--results_dir", type=str, default=None, help="default ../results/txt_only/ as in the reference")
    p.add_argument("--arch_layers", type=int, default=None, help="(testing) override encoder depth")
    p.add_argument("--max_grad_norm", type=float, default=None, help="clip the gradient to this global L2 norm before AdamW, as torch.nn.utils.clip_grad_norm_ (default: off)")
    return p


class SyntheticTexts(torch.utils.data.Dataset):
    """synthetic posts with the reference TxtOnly_Dataset item layout (models/datasets.py:49-75): ids / mask [T] (+ token_type_ids), one-hot
    target, data_id; right-padded to random lengths"""

    def __init__(self, n, vocab, num_labels, T, seed, txt_kind, pad_id, with_types, type_vocab):
        self.n, self.args = n, (vocab, num_labels, T, seed, txt_kind, pad_id, with_types, type_vocab)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        vocab, C, T, seed, kind, pad_id, with_types, type_vocab = self.args
        ids, mask, _, onehot = synthetic_batch(vocab, C, 1, T, seed * 1000003 + i, kind, pad_id, True, 2)
        item = {"ids": ids[0], "mask": mask[0]}
        if with_types:
            item["token_type_ids"] = torch.zeros(T, dtype=torch.int64)
        item["target"], item["data_id"] = onehot[0], torch.tensor(i)
        return item


def file_names(args, results_dir):
    """reference models/run_txt.py:57-63,75-76"""
    stem = results_dir + "{}_task{}_seed{}_".format(args.model_name, args.task, args.seed)
    return {"model": stem + "net.pth", "val": stem + "metrics_val.csv", "test": stem + "metrics_test.csv", "preds": stem + "preds.csv"}


def make_loaders(args, cfg, trainer):
    if cfg.data is not None and not args.synthetic:
        return trainer.load_data(cfg.data, testing=args.testing, eval_txt_test=args.eval_txt_test, task_name=cfg.task_name)
    a = trainer.model.arch
    n = 200 if args.testing else args.n_synthetic                        # --testing subsamples 200 rows (models/utils.py:135-138)
    mk = lambda cnt, seed: SyntheticTexts(cnt, a["vocab"], cfg.num_labels, cfg.max_length, seed, a["txt_kind"], a["pad_id"], trainer.with_types, a["type_vocab"])
    tr, va, te = mk(n, 11), mk(max(cfg.batch_size, n // 4), 1011), mk(max(cfg.batch_size, n // 4), 2011)
    dl = lambda ds, shuffle: torch.utils.data.DataLoader(ds, batch_size=cfg.batch_size, shuffle=shuffle, drop_last=False)
    labels = [int(tr[i]["target"].argmax()) for i in range(min(len(tr), 512))]
    return dl(tr, True), dl(va, False), dl(te, False), balanced_class_weights(labels, cfg.num_labels), None


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.use_loss_correction:
        raise NotImplementedError("--use_loss_correction is not part of this build")
    if mmdist.world_size() > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("run_txt is single-process: data-parallel training of the text-only path is not implemented "
                         f"(world size {max(mmdist.world_size(), int(os.environ.get('WORLD_SIZE', '1')))}); launch one process")
    from .text_only import TextModel
    torch.set_num_threads(max(1, int(os.environ.get("MMHIP_HOST_THREADS", "4"))))
    torch.manual_seed(args.seed)                      # models/run_txt.py:35-36
    np.random.seed(args.seed)
    results_dir = args.results_dir or results_dir_txt
    if args.testing:
        results_dir += "testing/"
    logger.info("Model: {}, Task: {}, Epochs: {}, LC:{}, seed: {}".format(args.model_name, args.task, args.epochs, args.use_loss_correction, args.seed))
    logger.info("Loading model and data")
    cfg = Config(args, multimodal=False, txt=True)
    kw = dict(dtype=args.dtype, seed=args.seed, max_grad_norm=args.max_grad_norm)
    if args.arch_layers:
        kw["arch"] = dict(layers=args.arch_layers)
    text_model = TextModel(cfg, args.model_name, **kw)
    train_loader, val_loader, test_loader, weight, txt_te_loader = make_loaders(args, cfg, text_model)
    names = file_names(args, results_dir)
    os.makedirs(results_dir, exist_ok=True)           # the reference requires the directory to pre-exist
    logger.info("Training")
    text_model.train(train_loader, val_loader, args.epochs, None, cfg.lr, cfg.weight_decay, te_dataloader=test_loader,
                     model_path=names["model"] if args.save_model else None, val_filename=names["val"], te_filename=names["test"], class_weight=weight)
    if args.save_preds:
        pred = text_model.eval(test_loader, class_weight=weight)
        pd.DataFrame({"data_id": pred["data_id"].tolist(), "label": pred["labels"].tolist(),
                      "prediction": pred["predictions"].tolist()}).to_csv(names["preds"], index=False)
        logger.info("%s saved", names["preds"])
    if args.eval_txt_test and txt_te_loader is not None:
        pred = text_model.eval(txt_te_loader, class_weight=weight)
        stem = names["preds"][: -len("preds.csv")]
        pd.DataFrame({"data_id": pred["data_id"].tolist(), "label": pred["labels"].tolist(),
                      "prediction": pred["predictions"].tolist()}).to_csv(stem + "preds_txt.csv", index=False)
        pd.DataFrame(compute_metrics(pred, cfg.num_labels)).to_csv(stem + "metrics_txt.csv", index=False)
    logger.info("Done!")


if __name__ == "__main__":
    main()
