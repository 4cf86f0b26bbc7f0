#!/usr/bin/env python3
"""The late-fusion train step (smtc_amd.mm_late.MMLate_Model.train_step) with --fusion_name aspect-att beside the same step with attention
fusion, at the config-2 shape (Bernice + ViT-B/16, B = 64, T = 128, bf16, no auxiliary loss), in ONE process on one box:

  * the attention step twice, before and after the aspect-att step: the difference of the two runs is the run-to-run spread the comparison
    has to be read against;
  * the aspect-att step;
  * the fusion operator's launches (mmhip_op_aspect_fusion_fwd, then _bwd: three kernels) under HIP events around ONE forward + backward
    sequence enqueued on an idle device, median over repetitions -- kernel time plus the launch gaps, as the step sees it; and both models'
    head chains measured as tools/txt_bench.py measures the attention one (forward: step spans; loss + backward stage 0: HIP events).

Prints and writes profiles/aspect_bench.txt.

    python tools/aspect_bench.py [--steps 20] [--warmup 5] [--layers 12]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import smtc_amd  # noqa: E402,F401
from smtc_amd import _lib  # noqa: E402
from smtc_amd.synthetic import synthetic_batch  # noqa: E402
from txt_bench import once_us, timed  # noqa: E402


def trainer(fusion, B, T, layers):
    from smtc_amd.mm_late import MMLate_Model
    cfg = types.SimpleNamespace(batch_size=B, num_labels=3, use_clip_loss=False, beta_itc=None, use_tim_loss=False, beta_itm=None, max_length=T, dropout=0.05)
    return MMLate_Model(cfg, "bernice", "vit", fusion, dtype="bf16", seed=0, arch=dict(layers_txt=layers, layers_img=layers))


def step_and_heads(fusion, B, T, layers, steps, warmup):
    """-> (ms/step, heads forward us, loss + heads backward us) of one freshly built model"""
    tr = trainer(fusion, B, T, layers)
    m, lib, s = tr.model, _lib.lib(), _lib.stream_ptr()
    a = m.arch
    ids, mask, pixels, onehot = synthetic_batch(a["vocab"], 3, B, T, 1, a["txt_kind"], a["pad_id"], False, a["image"], tr.device)
    n = [0]

    def one():
        n[0] += 1
        tr.train_step(ids, mask, pixels, onehot, None, 1e-5, 0.00025, n[0])
    ms = timed(one, steps, warmup)
    rows = []
    _lib.check(lib.mmhip_step_spans(m._handle, 1, None))
    for _ in range(6):
        one()
        buf = (ctypes.c_float * 5)()
        _lib.check(lib.mmhip_step_spans(m._handle, 1, buf))
        rows.append(list(buf))
    _lib.check(lib.mmhip_step_spans(m._handle, 0, None))
    heads_fwd_us = statistics.median(r[2] - max(r[0], r[1]) for r in rows[1:]) * 1e3
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
    del tr
    torch.cuda.empty_cache()
    return ms, heads_fwd_us, statistics.median(got)


def operator_us(B, H=768):
    lib, s, dev = _lib.lib(), _lib.stream_ptr(), "cuda:0"
    t_pool, v_pool = torch.tanh(torch.randn(B, H, device=dev)), torch.tanh(torch.randn(B, H, device=dev))
    a, b, d_feats = torch.randn(H, device=dev) * 0.05, torch.zeros(1, device=dev), torch.randn(B, H, device=dev)
    feats, w, e = torch.empty(B, H, device=dev), torch.empty(B, 2, device=dev), torch.empty(B, 2, device=dev)
    d_t, da, db = torch.zeros(B, H, device=dev), torch.zeros(H, device=dev), torch.zeros(1, device=dev)
    nws = int(lib.mmhip_op_aspect_fusion_ws_bytes(B, H))
    ws = torch.empty(nws // 4, device=dev)
    P = _lib.ptr

    def both():
        _lib.check(lib.mmhip_op_aspect_fusion_fwd(P(t_pool), P(v_pool), P(a), P(b), B, H, P(feats), P(w), P(e), s), "fwd")
        _lib.check(lib.mmhip_op_aspect_fusion_bwd(P(t_pool), P(v_pool), P(a), P(b), B, H, P(feats), P(w), P(e), P(d_feats), P(d_t), P(da), P(db), 0, 1,
                                                  P(ws), nws, s), "bwd")
    return once_us(both)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aspect_bench.txt"))
    args = ap.parse_args()
    B, T = args.batch, 128
    lines = [f"late-fusion train step, config 2 (Bernice + ViT-B/16, {args.layers} + {args.layers} layers), B = {B}, T = {T}, bf16, no auxiliary loss; "
             f"{torch.cuda.get_device_name(0)}"]
    runs = [("attention", "attention (first run)"), ("aspect-att", "aspect-att"), ("attention", "attention (second run)")]
    res = []
    for fusion, label in runs:
        ms, hf, hb = step_and_heads(fusion, B, T, args.layers, args.steps, args.warmup)
        res.append(ms)
        lines.append(f"{label:24s} {ms:8.3f} ms/step {B / ms * 1e3:9.1f} posts/s   head chain: forward {hf:7.1f} us + loss and backward stage 0 {hb:7.1f} us "
                     f"= {hf + hb:7.1f} us")
    spread = abs(res[0] - res[2])
    lines.append(f"run-to-run spread of the attention step: {spread:6.3f} ms; aspect-att minus the attention mean: {res[1] - 0.5 * (res[0] + res[2]):+7.3f} ms")
    lines.append(f"aspect-att fusion operator, forward + backward (three kernels) on an idle device (HIP events, median): {operator_us(B):7.1f} us")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
