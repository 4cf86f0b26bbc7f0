"""CPU: what the text-only and the image-only front ends must keep doing whatever code they share -- the trainers' epoch loop (prints, the order and
arguments of its calls, the CSV files, one save at the end) on trainers made without an engine, and the C entry points each model family resolves.
Every expectation is a literal of this file."""
import types

import numpy as np
import pandas as pd
import pytest
import torch

import smtc_amd  # noqa: F401
from smtc_amd import _lib

LR, WD, EPOCHS, LOG_EVERY = 3e-5, 0.125, 3, 2
WEIGHT = [1.0, 2.0, 0.5]
EVAL = {"val": dict(data_id=[0, 1, 2, 3], loss=0.5, predictions=[0, 1, 2, 1], labels=[0, 1, 1, 1]),
        "test": dict(data_id=[4, 5, 6], loss=0.25, predictions=[2, 2, 0], labels=[2, 1, 0])}

# three epochs of three batches (3, 3 and 2 rows), log_every = 2: iterations 0 and 2 of each epoch are logged, n is the batch's row count
STDOUT = "".join(f"{epoch}\nGot 2 / 3 with accuracy 66.67 loss 0.7500\nGot 2 / 2 with accuracy 100.00 loss 0.7500\nval\ntest\n" for epoch in range(3))
# epoch e, steps 3 e + 1 .. 3 e + 3; the overflow check follows a logged step only; each CSV is written after epochs 0 and 2 (even, and the last)
CALLS = [("step", 1), ("overflow",), ("step", 2), ("step", 3), ("overflow",), ("eval", "val"), ("csv", "val", 1), ("eval", "test"), ("csv", "test", 1),
         ("step", 4), ("overflow",), ("step", 5), ("step", 6), ("overflow",), ("eval", "val"), ("eval", "test"),
         ("step", 7), ("overflow",), ("step", 8), ("step", 9), ("overflow",), ("eval", "val"), ("csv", "val", 3), ("eval", "test"), ("csv", "test", 3),
         ("save", "net.pth")]
CSV = {"val": "metric,epoch-1,epoch-2,epoch-3\n"
              "f1_weighted,0.8500000000000001,0.8500000000000001,0.8500000000000001\n"
              "f1_macro,0.6,0.6,0.6\n"
              "precision_weighted,1.0,1.0,1.0\n"
              "precision_macro,0.6666666666666666,0.6666666666666666,0.6666666666666666\n"
              "recall_weighted,0.75,0.75,0.75\n"
              "recall_macro,0.5555555555555556,0.5555555555555556,0.5555555555555556\n"
              "loss,0.5,0.5,0.5\n",
       "test": "metric,epoch-1,epoch-2,epoch-3\n"
               "f1_weighted,0.5555555555555556,0.5555555555555556,0.5555555555555556\n"
               "f1_macro,0.5555555555555556,0.5555555555555556,0.5555555555555556\n"
               "precision_weighted,0.5,0.5,0.5\n"
               "precision_macro,0.5,0.5,0.5\n"
               "recall_weighted,0.6666666666666666,0.6666666666666666,0.6666666666666666\n"
               "recall_macro,0.6666666666666666,0.6666666666666666,0.6666666666666666\n"
               "loss,0.25,0.25,0.25\n"}

ROWS = (3, 3, 2)
ONEHOT = [torch.eye(3, dtype=torch.int64)[[0, 1, 2]], torch.eye(3, dtype=torch.int64)[[2, 2, 0]], torch.eye(3, dtype=torch.int64)[[1, 0]]]
# text: every item is padded to 96 columns; its longest post has 20, 40 and 70 tokens, so _batch hands the step 32, 64 and 96 columns
T_PAD, LONGEST, T_STEP = 96, (20, 40, 70), (32, 64, 96)


def _text_batches():
    g, out = torch.Generator().manual_seed(0), []
    for n, longest, onehot in zip(ROWS, LONGEST, ONEHOT):
        lengths = [longest] + [5 + 3 * r for r in range(1, n)]
        mask = torch.zeros(n, T_PAD, dtype=torch.int64)
        for r, length in enumerate(lengths):
            mask[r, :length] = 1
        ids = torch.randint(3, 50, (n, T_PAD), generator=g) * mask + (1 - mask)
        tt = (torch.arange(T_PAD).expand(n, T_PAD) >= 4).long() * mask
        out.append({"ids": ids, "mask": mask, "token_type_ids": tt, "target": onehot, "data_id": torch.arange(n)})
    return out


def _image_batches():
    g = torch.Generator().manual_seed(1)
    return [{"pixel_values": torch.rand(n, 1, 3, 4, 4, generator=g), "labels": onehot, "data_id": torch.arange(n)} for n, onehot in zip(ROWS, ONEHOT)]


def _run_epochs(trainer, batches, monkeypatch, tmp_path, capsys):
    """the trainer's own train() over `batches` with recorders in place of everything that needs an engine -> (calls, step arguments, stdout, paths)"""
    calls, steps = [], []
    loaders = {"val": [{"which": "val"}], "test": [{"which": "test"}]}
    paths = {"val": str(tmp_path / "val.csv"), "test": str(tmp_path / "test.csv"), "model": str(tmp_path / "net.pth")}
    loss_fn = torch.nn.CrossEntropyLoss(weight=torch.tensor(WEIGHT))

    def train_step(*args):
        calls.append(("step", args[-1]))
        steps.append(args)
        return torch.tensor([0.75]), torch.tensor([2], dtype=torch.int32)

    def evaluate(loader, class_weight=None):
        which = next(k for k, v in loaders.items() if v is loader)
        assert class_weight is loss_fn.weight
        calls.append(("eval", which))
        r = EVAL[which]
        return {"data_id": np.array(r["data_id"]), "loss": r["loss"], "predictions": np.array(r["predictions"]), "labels": np.array(r["labels"])}

    to_csv = pd.DataFrame.to_csv

    def csv(frame, fname, **kw):
        calls.append(("csv", next(k for k, v in paths.items() if v == fname), len(frame.columns) - 1))
        return to_csv(frame, fname, **kw)

    monkeypatch.setattr(trainer, "train_step", train_step)
    monkeypatch.setattr(trainer, "eval", evaluate)
    monkeypatch.setattr(trainer, "check_overflow", lambda: calls.append(("overflow",)))
    monkeypatch.setattr(trainer, "save_model", lambda path: calls.append(("save", path[len(str(tmp_path)) + 1:])))
    monkeypatch.setattr(pd.DataFrame, "to_csv", csv)
    capsys.readouterr()
    trainer.train(batches, loaders["val"], EPOCHS, loss_fn=loss_fn, lr=LR, weight_decay=WD, te_dataloader=loaders["test"], model_path=paths["model"],
                  val_filename=paths["val"], te_filename=paths["test"], log_every=LOG_EVERY)
    return calls, steps, capsys.readouterr().out, paths, loss_fn


def _bare(cls, **attrs):
    """a trainer without an engine: only what the epoch loop reads"""
    t = object.__new__(cls)
    t.device, t.num_labels, t.model = torch.device("cpu"), 3, types.SimpleNamespace()
    for k, v in attrs.items():
        setattr(t, k, v)
    return t


def _check_run(calls, out, paths):
    assert out == STDOUT
    assert calls == CALLS
    for which in ("val", "test"):
        with open(paths[which]) as f:
            assert f.read() == CSV[which], which


@pytest.mark.parametrize("with_types", [True, False])
def test_text_epoch_loop(with_types, monkeypatch, tmp_path, capsys):
    from smtc_amd.text_only import TextModel
    batches = _text_batches()
    calls, steps, out, paths, loss_fn = _run_epochs(_bare(TextModel, with_types=with_types), batches, monkeypatch, tmp_path, capsys)
    _check_run(calls, out, paths)
    assert len(steps) == 9
    for k, args in enumerate(steps):
        ids, mask, tt, onehot, cw, lr, wd, step = args
        b, t = batches[k % 3], T_STEP[k % 3]
        assert tuple(ids.shape) == tuple(mask.shape) == (ROWS[k % 3], t)
        assert torch.equal(ids, b["ids"][:, :t]) and torch.equal(mask, b["mask"][:, :t]) and int(b["mask"][:, t:].sum()) == 0
        if with_types:
            assert torch.equal(tt, b["token_type_ids"][:, :t]) and int(tt.sum()) > 0
        else:
            assert tt is None
        assert onehot is b["target"] and cw is loss_fn.weight and cw.tolist() == WEIGHT
        assert (lr, wd, step) == (LR, WD, k + 1)


def test_image_epoch_loop(monkeypatch, tmp_path, capsys):
    from smtc_amd.image_only import ImageModel
    batches = _image_batches()
    calls, steps, out, paths, loss_fn = _run_epochs(_bare(ImageModel), batches, monkeypatch, tmp_path, capsys)
    _check_run(calls, out, paths)
    assert len(steps) == 9
    for k, args in enumerate(steps):
        pixels, onehot, cw, lr, wd, step = args
        b = batches[k % 3]
        assert pixels is b["pixel_values"] and onehot is b["labels"] and cw is loss_fn.weight and cw.tolist() == WEIGHT
        assert (lr, wd, step) == (LR, WD, k + 1)


TXT_ABI = dict(create="mmhip_txt_create", destroy="mmhip_txt_destroy", param_count="mmhip_txt_param_count", param_info_at="mmhip_txt_param_info_at",
               workspace_bytes="mmhip_txt_workspace_bytes", num_stages="mmhip_num_backward_stages", stage_grad_range="mmhip_stage_grad_range")
IMG_ABI = dict(create="mmhip_img_create", destroy="mmhip_img_destroy", param_count="mmhip_img_param_count", param_info_at="mmhip_img_param_info_at",
               workspace_bytes="mmhip_img_workspace_bytes", num_stages="mmhip_num_backward_stages", stage_grad_range="mmhip_stage_grad_range")


def test_entry_point_names():
    """the seven entry points the engine module resolves by name for each family (a handle of either is read through the two shared stage calls)"""
    from smtc_amd.image_only import ViTClassifier
    from smtc_amd.text_only import BERNICE, BERT
    assert dict(BERT._ABI) == dict(BERNICE._ABI) == TXT_ABI
    assert dict(ViTClassifier._ABI) == IMG_ABI
    for abi in (TXT_ABI, IMG_ABI):
        assert len(abi) == 7 and all(name in _lib.EXPORTS for name in abi.values())
