#!/usr/bin/env python3
"""Text-only train step (smtc_amd.text_only.TextModel.train_step) at the Bernice shape, B = 64, T = 128, in bf16 and bf16x3: ms/step and posts/s.
Beside it, on the same box and in the same process:

  * the fused CLS head's two launches (mmhip_op_cls_head_fwd with the loss, mmhip_op_cls_head_bwd): HIP events around ONE forward + backward
    pair enqueued on an idle device, median over repetitions -- kernel time plus the launch gap between the two, as the step sees it;
  * the late-fusion head chain of a config-2 model (Bernice + ViT-B/16, attention fusion, no auxiliary loss) at the same B / T: its forward part
    from mmhip_step_spans of the fused step (forward end - the later tower end), its loss + backward part (mmhip_loss, mmhip_backward_stage 0)
    under HIP events around one such sequence enqueued on an idle device, median over repetitions;
  * the late-fusion step's text-tower-plus-backward share (text tower end + backward end - forward end of the same spans): the number the
    text-only step is set against.

Prints and writes profiles/txt_bench.txt.

    python tools/txt_bench.py [--steps 20] [--warmup 5] [--layers 12]
"""
import argparse
import ctypes
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import smtc_amd  # noqa: E402,F401
from smtc_amd import _lib  # noqa: E402
from smtc_amd.synthetic import synthetic_batch  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def once_us(fn, reps=21, warmup=3):
    """median HIP-event duration (us) of ONE call of fn enqueued on an idle device"""
    got = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            got.append(a.elapsed_time(b) * 1e3)
    return statistics.median(got)


def step_ms(dtype, B, T, layers, steps, warmup):
    from smtc_amd.text_only import TextModel

    class Cfg:
        batch_size, num_labels, max_length, dropout, use_loss_correction = B, 3, T, 0.05, False
    tm = TextModel(Cfg, "bernice", arch=dict(layers=layers), dtype=dtype, seed=0)
    a = tm.model.arch
    ids, mask, _, onehot = synthetic_batch(a["vocab"], 3, B, T, 1, a["txt_kind"], a["pad_id"], False, 2, tm.device)
    n = [0]

    def one():
        n[0] += 1
        tm.train_step(ids, mask, None, onehot, None, 1e-5, 0.00025, n[0])
    ms = timed(one, steps, warmup)
    del tm
    torch.cuda.empty_cache()
    return ms


def head_us(B, C=3, H=768):
    lib, s, dev = _lib.lib(), _lib.stream_ptr(), "cuda:0"
    x = torch.randn(B * H, device=dev).to(torch.bfloat16)
    W, b = torch.randn(C, H, device=dev) * 0.02, torch.zeros(C, device=dev)
    onehot = torch.eye(C, dtype=torch.int64, device=dev)[torch.randint(0, C, (B,), device=dev)]
    logits, dl = torch.empty(B, C, device=dev), torch.empty(B, C, device=dev)
    loss, nc = torch.empty(1, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    dW, db, dx = torch.zeros(C, H, device=dev), torch.zeros(C, device=dev), torch.empty(B * H, dtype=torch.bfloat16, device=dev)

    def both():
        _lib.check(lib.mmhip_op_cls_head_fwd(_lib.BF16, _lib.ptr(x), H, _lib.ptr(W), _lib.ptr(b), B, C, H, 0.05, 1, _lib.ptr(logits), _lib.ptr(onehot), None,
                                             _lib.ptr(loss), _lib.ptr(nc), _lib.ptr(dl), s), "fwd")
        _lib.check(lib.mmhip_op_cls_head_bwd(_lib.BF16, _lib.ptr(x), H, _lib.ptr(W), _lib.ptr(dl), B, C, H, 0.05, 1, _lib.ptr(dW), _lib.ptr(db), _lib.BF16,
                                             _lib.ptr(dx), H, 1.0, 0, s), "bwd")
    return once_us(both)


def late_fusion(B, T, layers):
    """config-2 late-fusion model at the same B / T: (heads forward us, loss + heads backward us, text tower + backward share ms, step ms)"""
    from smtc_amd.mm_late import MMLate_Model
    C = 3
    cfg = types.SimpleNamespace(batch_size=B, num_labels=C, use_clip_loss=False, beta_itc=None, use_tim_loss=False, beta_itm=None, max_length=T, dropout=0.05)
    tr = MMLate_Model(cfg, "bernice", "vit", "attention", dtype="bf16", seed=0, arch=dict(layers_txt=layers, layers_img=layers))
    m, lib, s = tr.model, _lib.lib(), _lib.stream_ptr()
    a = m.arch
    ids, mask, pixels, onehot = synthetic_batch(a["vocab"], C, B, T, 1, a["txt_kind"], a["pad_id"], False, a["image"], tr.device)
    n = 0
    for _ in range(3):
        n += 1
        tr.train_step(ids, mask, pixels, onehot, None, 1e-5, 0.00025, n)
    # phase ends of the fused step: [0] image tower, [1] text tower, [2] forward, [3] backward, [4] step, ms after the forward's fork
    rows = []
    _lib.check(lib.mmhip_step_spans(m._handle, 1, None))
    for _ in range(6):
        n += 1
        tr.train_step(ids, mask, pixels, onehot, None, 1e-5, 0.00025, n)
        buf = (ctypes.c_float * 5)()
        _lib.check(lib.mmhip_step_spans(m._handle, 1, buf))
        rows.append(list(buf))
    _lib.check(lib.mmhip_step_spans(m._handle, 0, None))
    rows = rows[1:]
    heads_fwd_us = statistics.median(r[2] - max(r[0], r[1]) for r in rows) * 1e3
    share_ms = statistics.median(r[1] + r[3] - r[2] for r in rows)
    step = statistics.median(r[4] for r in rows)
    # loss + backward stage 0 (the heads) of the staged path, then the rest of the backward so that the handle and the gradient end clean
    w_cls, w_itc, w_itm = tr.loss_weights()
    lo = torch.empty(4, device=tr.device)
    got = []
    m.train()
    for i in range(12):
        m._engine_forward(ids, mask, pixels)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(lib.mmhip_loss(m._handle, _lib.ptr(onehot), None, None, w_cls, w_itc, w_itm, _lib.ptr(lo), None, s), "loss")
        _lib.check(lib.mmhip_backward_begin(m._handle, None, None, None, None, s), "backward_begin")
        _lib.check(lib.mmhip_backward_stage(m._handle, 0, s), "backward_stage")
        e1.record()
        for st in range(1, lib.mmhip_num_backward_stages(m._handle)):
            _lib.check(lib.mmhip_backward_stage(m._handle, st, s), "backward_stage")
        _lib.check(lib.mmhip_backward_finish(m._handle, s), "backward_finish")
        torch.cuda.synchronize()
        m._flat_grad.zero_()
        m._word_row_state.bitwise_and_(0xFE)
        if i >= 3:
            got.append(e0.elapsed_time(e1) * 1e3)
    return heads_fwd_us, statistics.median(got), share_ms, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "txt_bench.txt"))
    args = ap.parse_args()
    B, T = args.batch, 128
    lines = [f"text-only train step, Bernice shape ({args.layers} layers, vocab 250002), B = {B}, T = {T}; {torch.cuda.get_device_name(0)}"]
    for dt in ("bf16", "bf16x3"):
        ms = step_ms(dt, B, T, args.layers, args.steps, args.warmup)
        lines.append(f"{dt:7s} {ms:8.3f} ms/step {B / ms * 1e3:9.1f} posts/s")
    lines.append(f"fused CLS head, forward(+loss) + backward, one pair of launches on an idle device (HIP events, median): {head_us(B):7.1f} us")
    hf, hb, share, step = late_fusion(B, T, args.layers)
    lines.append(f"late-fusion head chain (config 2, bf16, same B / T): forward {hf:7.1f} us (step spans: forward end - later tower end) + "
                 f"loss and backward stage 0 {hb:7.1f} us (HIP events, one sequence on an idle device, median) = {hf + hb:7.1f} us")
    lines.append(f"late-fusion config-2 step (bf16): {step:8.3f} ms; its text tower + backward share (text tower end + backward end - forward end): {share:8.3f} ms")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
