"""Command line of the image-only runs -- same flags, defaults, file names and CSV layouts as the reference's models/run_img.py:19-92.
Additive flags: --synthetic / --n_synthetic (no dataset on disk), --dtype, --batch_size, --results_dir, --arch_layers, --max_grad_norm.  Single process.
`--model_name vit` is what this build trains; beit, deit, the resnets, --conv_att and --feature_extract are refused.

    python -m smtc_amd.run_img --model_name vit --task 3 --testing
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
from .config import Config, results_dir_img
from .utils import balanced_class_weights

logging.basicConfig(format="%(asctime)s - %(message)s", datefmt="%Y-%m-%d %H:%M:%S", level=logging.INFO)
logger = logging.getLogger(__name__)


def build_parser():
    p = argparse.ArgumentParser(description="run image-only models")
    # reference flags, models/run_img.py:20-31 (names, types, choices, defaults unchanged)
    p.add_argument("--model_name", type=str, choices=["vit", "beit", "deit", "resnet50", "resnet152"], help="model name")
    p.add_argument("--conv_att", action="store_true", help="CNN ATT")
    p.add_argument("--feature_extract", action="store_true", help="feature_extract")
    p.add_argument("--task", type=int, choices=[0, 1, 2, 3, 4, 5, 6], help="task to run")
    p.add_argument("--epochs", type=int, default=2, help="number of epochs")
    p.add_argument("--weight_decay", type=float, default=0.00025, help="weight decay param")
    p.add_argument("--lr", type=float, default=1e-5, help="learning rate param")
    p.add_argument("--dropout", type=float, default=0.05, help="dropout param (as in the reference, never applied on the vit branch)")
    p.add_argument("--seed", type=int, default=30, help="manual seed")
    p.add_argument("--testing", action="store_true", help="testing sample")
    p.add_argument("--save_model", action="store_true", help="eval test")
    p.add_argument("--save_preds", action="store_true", help="eval test")
    # additive
    p.add_argument("--batch_size", type=int, default=None, help="batch size (default: the reference's per-task value)")
    p.add_argument("--synthetic", action="store_true", help="synthetic images instead of the data key")
    p.add_argument("--n_synthetic", type=int, default=256, help="synthetic training images")
    p.add_argument("--dtype", choices=["bf16", "f16", "bf16x3"], default="bf16", help="bf16x3 = strict-parity mode (fp32 activations, 3 bf16 MFMA products per Linear)")
    p.add_argument("--results_dir", type=str, default=None, help="default ../results/img_only/ as in the reference")
    p.add_argument("--arch_layers", type=int, default=None, help="(testing) override encoder depth")
    p.add_argument("--max_grad_norm", type=float, default=None, help="clip the gradient to this global L2 norm before AdamW, as torch.nn.utils.clip_grad_norm_ (default: off)")
    return p


def check_supported(args):
    """what this build does not train is refused, as the other command lines here refuse what they do not build"""
    if args.model_name != "vit":
        raise NotImplementedError(f"--model_name {args.model_name}: the image-only path builds `vit`; beit, deit and the resnets are not part of this build")
    if args.conv_att or args.feature_extract:
        raise NotImplementedError("--conv_att / --feature_extract belong to the reference's CNN models, which are not part of this build")


class SyntheticImages(torch.utils.data.Dataset):
    """synthetic images with the reference ImgOnly_Dataset item layout (models/datasets.py:64-91): pixel_values [1, 3, S, S] uniform in (-1, 1)
    (the range of the ViT feature extractor's output), one-hot labels, data_id"""

    def __init__(self, n, num_labels, image, seed):
        self.n, self.num_labels, self.image, self.seed = n, num_labels, image, seed

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 1000003 + i)
        px = torch.rand(1, 3, self.image, self.image, generator=g) * 2 - 1
        label = int(torch.randint(0, self.num_labels, (1,), generator=g))
        return {"pixel_values": px, "labels": torch.nn.functional.one_hot(torch.tensor(label), self.num_labels).to(torch.int64), "data_id": torch.tensor(i)}


def file_names(args, results_dir):
    """reference models/run_img.py:58-67,84-85"""
    stem = results_dir + "{}_task{}_seed{}_".format(args.model_name, args.task, args.seed)
    return {"model": stem + "net.pth", "val": stem + "metrics_val.csv", "test": stem + "metrics_test.csv", "preds": stem + "preds.csv"}


def make_loaders(args, cfg, trainer):
    if cfg.data is not None and not args.synthetic:
        return trainer.load_data(cfg.data, cfg.img_fmt, testing=args.testing, task_name=cfg.task_name)
    n = 200 if args.testing else args.n_synthetic                        # --testing subsamples 200 rows (models/utils.py:135-138)
    mk = lambda cnt, seed: SyntheticImages(cnt, cfg.num_labels, trainer.model.arch["image"], seed)
    tr, va, te = mk(n, 11), mk(max(cfg.batch_size, n // 4), 1011), mk(max(cfg.batch_size, n // 4), 2011)
    dl = lambda ds: torch.utils.data.DataLoader(ds, batch_size=cfg.batch_size)
    labels = [int(tr[i]["labels"].argmax()) for i in range(min(len(tr), 512))]
    return dl(tr), dl(va), dl(te), balanced_class_weights(labels, cfg.num_labels)


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_supported(args)
    if mmdist.world_size() > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("run_img is single-process: data-parallel training of the image-only path is not implemented "
                         f"(world size {max(mmdist.world_size(), int(os.environ.get('WORLD_SIZE', '1')))}); launch one process")
    from .image_only import ImageModel
    torch.set_num_threads(max(1, int(os.environ.get("MMHIP_HOST_THREADS", "4"))))
    torch.manual_seed(args.seed)                      # models/run_img.py:35-36
    np.random.seed(args.seed)
    results_dir = args.results_dir or results_dir_img
    if args.testing:
        results_dir += "testing/"
    logger.info("Model: {}, Task: {}, feature extract: {}, conv att: {}, Epochs: {}, seed: {}".format(
        args.model_name, args.task, args.feature_extract, args.conv_att, args.epochs, args.seed))
    logger.info("Loading model and data")
    cfg = Config(args, multimodal=False)
    kw = dict(dtype=args.dtype, seed=args.seed, max_grad_norm=args.max_grad_norm)
    if args.arch_layers:
        kw["arch"] = dict(layers=args.arch_layers)
    image_model = ImageModel(cfg.batch_size, cfg.num_labels, args.model_name, conv_att=args.conv_att, feature_extract=args.feature_extract, **kw)
    train_loader, val_loader, test_loader, weight = make_loaders(args, cfg, image_model)
    names = file_names(args, results_dir)
    os.makedirs(results_dir, exist_ok=True)           # the reference requires the directory to pre-exist
    logger.info("Training")
    image_model.train(train_loader, val_loader, args.epochs, None, cfg.lr, cfg.weight_decay, te_dataloader=test_loader,
                      model_path=names["model"] if args.save_model else None, val_filename=names["val"], te_filename=names["test"], class_weight=weight)
    logger.info("{} saved!".format(names["val"]))
    if args.save_preds:
        logger.info("Evaluate and compute metrics")
        pred = image_model.eval(test_loader, class_weight=weight)
        pd.DataFrame({"data_id": pred["data_id"].tolist(), "label": pred["labels"].tolist(),
                      "prediction": pred["predictions"].tolist()}).to_csv(names["preds"], index=False)
        logger.info("%s saved", names["preds"])
    logger.info("Done!")


if __name__ == "__main__":
    main()
