#!/usr/bin/env python3
"""Image-only train step (smtc_amd.image_only.ImageModel.train_step): full ViT-B/16 at 224 px, B = 16 (the reference's batch size) and B = 64, in
bf16 and bf16x3 -- ms/step (median of per-step HIP-event times after a warm-up), images/s and the matrix-product FLOP rate from the shapes.
Beside it, on the same box and in the same process:

  * the text-only step of tools/txt_bench.py (Bernice shape, B = 64, T = 128, bf16) with its FLOP rate under the same formula: the layers have the
    same widths, so the two rates should be close;
  * the phase ends of the image step from mmhip_step_spans (tower forward, head, backward, optimizer tail);
  * launch_vit_embed_bwd alone (mmhip_op_vit_embed_bwd): us and bytes/s against the HBM peak (8.0 TB/s spec, about 6.3 TB/s achievable);
  * the long attention backward alone (mmhip_op_attn_bwd_long) at the step's shape: us per call, times the layers, as a share of the step.

FLOPs counted: 2 M N K per matrix product -- per layer the four Linears forward and twice that backward (dX and dW), attention's 2 products
forward and 5 backward of 2 S^2 64 each per head and post, the patch projection forward and its weight gradient (text: no patch projection).

Prints and writes profiles/img_bench.txt.

    python tools/img_bench.py [--steps 15] [--warmup 5] [--layers 12]
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import smtc_amd  # noqa: E402,F401
from smtc_amd import _lib  # noqa: E402
from smtc_amd.synthetic import synthetic_batch  # noqa: E402

HBM_PEAK = 8.0e12


def per_step_ms(fn, steps, warmup):
    """median over `steps` of the HIP-event time of one call, back to back after `warmup` calls"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return statistics.median(ev[i].elapsed_time(ev[i + 1]) for i in range(steps))


def once_us(fn, reps=21, warmup=3):
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


def step_flops(B, S, layers, H=768, I=3072, patch_k=0):
    M = B * S
    linear = 2.0 * M * (3 * H * H + H * H + 2 * H * I)
    attn = 2.0 * B * (H // 64) * S * S * 64
    f = layers * (3 * linear + 7 * attn)
    if patch_k:
        f += 2 * 2.0 * B * (S - 1) * H * patch_k
    return f


def image_step(dtype, B, layers, steps, warmup, spans=False):
    from smtc_amd.image_only import ImageModel
    tm = ImageModel(B, 3, "vit", arch=dict(layers=layers), dtype=dtype, seed=0)
    g = torch.Generator().manual_seed(1)
    px = (torch.rand(B, 3, 224, 224, generator=g) * 2 - 1).to(tm.device)
    onehot = torch.eye(3, dtype=torch.int64)[torch.randint(0, 3, (B,), generator=g)].to(tm.device)
    n = [0]

    def one():
        n[0] += 1
        tm.train_step(px, onehot, None, 1e-5, 0.00025, n[0])
    ms = per_step_ms(one, steps, warmup)
    rows = []
    if spans:
        lib = _lib.lib()
        _lib.check(lib.mmhip_step_spans(tm.model._handle, 1, None))
        for _ in range(6):
            one()
            buf = (ctypes.c_float * 5)()
            _lib.check(lib.mmhip_step_spans(tm.model._handle, 1, buf))
            rows.append(list(buf))
        _lib.check(lib.mmhip_step_spans(tm.model._handle, 0, None))
        rows = rows[1:]
    del tm
    torch.cuda.empty_cache()
    return ms, rows


def text_step(B, T, layers, steps, warmup):
    from smtc_amd.text_only import TextModel

    class Cfg:
        batch_size, num_labels, max_length, dropout, use_loss_correction = B, 3, T, 0.05, False
    tm = TextModel(Cfg, "bernice", arch=dict(layers=layers), dtype="bf16", seed=0)
    a = tm.model.arch
    ids, mask, _, onehot = synthetic_batch(a["vocab"], 3, B, T, 1, a["txt_kind"], a["pad_id"], False, 2, tm.device)
    n = [0]

    def one():
        n[0] += 1
        tm.train_step(ids, mask, None, onehot, None, 1e-5, 0.00025, n[0])
    ms = per_step_ms(one, steps, warmup)
    del tm
    torch.cuda.empty_cache()
    return ms


def embed_bwd_us(B, P=197, H=768):
    lib, s, dev = _lib.lib(), _lib.stream_ptr(), "cuda:0"
    dx = torch.randn(B * P * H, device=dev).to(torch.bfloat16)
    dpos, dcls = torch.zeros(P * H, device=dev), torch.zeros(H, device=dev)
    dpe = torch.empty(B * (P - 1) * H, dtype=torch.bfloat16, device=dev)
    need = lib.mmhip_op_vit_embed_bwd_ws_bytes(B, P, H)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    us = once_us(lambda: _lib.check(lib.mmhip_op_vit_embed_bwd(_lib.BF16, _lib.ptr(dx), B, P, H, 1.0, _lib.ptr(dpos), _lib.ptr(dcls), _lib.ptr(dpe), 0,
                                                                _lib.ptr(ws), need, s), "vit_embed_bwd"))
    nbytes = B * P * H * 2 + B * (P - 1) * H * 2 + 2 * (P + 1) * H * 4 + 2 * need
    return us, nbytes


def attn_bwd_us(B, P=197, heads=12):
    lib, s, dev = _lib.lib(), _lib.stream_ptr(), "cuda:0"
    H = heads * 64
    qkv = (0.5 * torch.randn(B * P, 3 * H, device=dev)).to(torch.bfloat16)
    ctx = torch.empty(B * P, H, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B * heads * P, device=dev)
    _lib.check(lib.mmhip_op_attn_fwd(_lib.BF16, _lib.ptr(qkv), None, _lib.ptr(ctx), _lib.ptr(lse), B, P, heads, 0.0, 0, 0, s), "attn_fwd")
    dctx = (0.1 * torch.randn(B * P, H, device=dev)).to(torch.bfloat16)
    dqkv = torch.empty_like(qkv)
    return once_us(lambda: _lib.check(lib.mmhip_op_attn_bwd_long(_lib.BF16, _lib.ptr(qkv), None, _lib.ptr(ctx), _lib.ptr(dctx), _lib.ptr(lse), _lib.ptr(dqkv),
                                                                 B, P, heads, 0.0, 0, 0, s), "attn_bwd_long"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "img_bench.txt"))
    args = ap.parse_args()
    L = args.layers
    lines = [f"image-only train step, ViT-B/16 ({L} layers) at 224 px (197 tokens); median of {args.steps} per-step HIP-event times after {args.warmup} warm-up "
             f"steps; {torch.cuda.get_device_name(0)}"]
    step_at = {}
    for B in (16, 64):
        for dt in ("bf16", "bf16x3"):
            ms, rows = image_step(dt, B, L, args.steps, args.warmup, spans=(dt == "bf16"))
            fl = step_flops(B, 197, L, patch_k=768)
            step_at[(B, dt)] = ms
            lines.append(f"B = {B:3d} {dt:7s} {ms:8.3f} ms/step {B / ms * 1e3:9.1f} images/s {fl / ms * 1e-9:8.1f} TFLOP/s (matrix products, {fl * 1e-12:.2f} TFLOP per step)")
            if rows:
                med = lambda i: statistics.median(r[i] for r in rows)
                lines.append(f"          phase ends after the step's start (mmhip_step_spans, ms): tower forward {med(0):.3f}, head {med(2):.3f}, backward + layer "
                             f"optimizers {med(3):.3f}, step {med(4):.3f}")
    tms = text_step(64, 128, L, args.steps, args.warmup)
    tfl = step_flops(64, 128, L)
    lines.append(f"text-only step (Bernice shape, B = 64, T = 128, bf16, same process): {tms:8.3f} ms/step {tfl / tms * 1e-9:8.1f} TFLOP/s under the same formula "
                 f"(its CLS-only last layer does less than the formula counts)")
    for B in (16, 64):
        us, nbytes = embed_bwd_us(B)
        lines.append(f"launch_vit_embed_bwd alone, B = {B}, bf16: {us:7.1f} us, {nbytes * 1e-6:.1f} MB moved, {nbytes / us * 1e-6:.2f} TB/s = "
                     f"{nbytes / us * 1e6 / HBM_PEAK * 100:.0f} % of the 8.0 TB/s HBM peak (one call on an idle device, HIP events, median)")
        au = attn_bwd_us(B)
        lines.append(f"launch_attn_bwd_long alone, B = {B}, bf16: {au:7.1f} us per call, x {L} layers = {au * L * 1e-3:.3f} ms = "
                     f"{au * L * 1e-3 / step_at[(B, 'bf16')] * 100:.1f} % of the bf16 step")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
