#!/usr/bin/env python3
"""What global-norm gradient clipping (max_grad_norm) costs in the late-fusion train step, at the config-2 shape (Bernice + ViT-B/16, B = 64, T = 128,
bf16, attention fusion, no auxiliary loss), in ONE process on one box, the four arms taken in turn round after round on ONE trainer:

  (a) the default step (each text layer's AdamW beside the backward);
  (b) MMHIP_EARLY_ADAMW=0: every AdamW launch after the backward -- the order an armed clip imposes;
  (c) armed with a threshold that never clips (1e9);
  (d) armed and clipping (1e-3).

(c) - (b) is the price of the norm itself, (b) - (a) the price of the launch order; the spread of (a) over the rounds is what both are read against.
Then the three norm launches alone, on an idle device (HIP events, median), with the bytes they read and the rate, beside the AdamW launches over
the same ranges in the same process (bytes read + written): the yardstick for a kernel that streams the same buffer.

Prints and writes profiles/grad_clip_bench.txt (appending: the digests and the parent A/B of the unarmed path are written to the same file).

    python tools/clip_bench.py [--steps 10] [--warmup 3] [--rounds 5] [--layers 12]
"""
import argparse
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import smtc_amd  # noqa: E402,F401
from smtc_amd.synthetic import synthetic_batch  # noqa: E402
from txt_bench import once_us, timed  # noqa: E402

ARMS = (("a", "default step", None, None), ("b", "MMHIP_EARLY_ADAMW=0", "0", None), ("c", "armed, max_grad_norm 1e9 (never clips)", None, 1e9),
        ("d", "armed, max_grad_norm 1e-3 (clips)", None, 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_clip_bench.txt"))
    args = ap.parse_args()
    from smtc_amd.mm_late import MMLate_Model
    B, T, L = args.batch, 128, args.layers
    cfg = types.SimpleNamespace(batch_size=B, num_labels=3, use_clip_loss=False, beta_itc=None, use_tim_loss=False, beta_itm=None, max_length=T, dropout=0.05)
    tr = MMLate_Model(cfg, "bernice", "vit", "attention", dtype="bf16", seed=0, arch=dict(layers_txt=L, layers_img=L))
    m = tr.model
    a = m.arch
    ids, mask, pixels, onehot = synthetic_batch(a["vocab"], 3, B, T, 1, a["txt_kind"], a["pad_id"], False, a["image"], tr.device)
    n = [0]

    def one():
        n[0] += 1
        tr.train_step(ids, mask, pixels, onehot, None, 1e-5, 0.00025, n[0])

    ms = {k: [] for k, *_ in ARMS}
    stats = {}
    for _ in range(args.rounds):
        for key, _, early, max_norm in ARMS:
            os.environ.pop("MMHIP_EARLY_ADAMW", None)
            if early is not None:
                os.environ["MMHIP_EARLY_ADAMW"] = early
            tr.set_max_grad_norm(max_norm)
            ms[key].append(timed(one, args.steps, args.warmup))
            if max_norm is not None:
                stats[key] = tr.grad_clip_stats()
    os.environ.pop("MMHIP_EARLY_ADAMW", None)
    tr.set_max_grad_norm(None)
    med = {k: statistics.median(v) for k, v in ms.items()}
    lines = [f"late-fusion train step, config-2 shape (Bernice + ViT-B/16, {L} + {L} layers), B = {B}, T = {T}, bf16, attention fusion, no auxiliary loss; "
             f"{torch.cuda.get_device_name(0)}; one trainer, {args.rounds} rounds of the four arms in turn, {args.warmup} + {args.steps} steps each"]
    for key, label, _, _ in ARMS:
        lines.append(f"({key}) {label:42s} median {med[key]:8.3f} ms/step  min {min(ms[key]):8.3f}  max {max(ms[key]):8.3f}   rounds " +
                     " ".join(f"{x:.3f}" for x in ms[key]))
    lines.append(f"run-to-run spread of (a): {max(ms['a']) - min(ms['a']):.3f} ms over {args.rounds} rounds")
    lines.append(f"(b) - (a), the launch order (no per-layer AdamW beside the backward): {med['b'] - med['a']:+.3f} ms/step")
    lines.append(f"(c) - (b), the norm itself (three launches + the coefficient read by every AdamW launch): {med['c'] - med['b']:+.3f} ms/step")
    lines.append(f"(d) - (c), clipping versus not clipping: {med['d'] - med['c']:+.3f} ms/step")
    for key in ("c", "d"):
        lines.append(f"({key}) last step: {stats[key]}")

    # the norm launches alone, beside AdamW over the same ranges: a gradient with every dense element and B * T word rows set
    ranges = m.active_ranges(False, False)
    word = m._word_info
    w0, (V, H) = word["offset"], word["shape"]
    dense = sum(min(e, w0) - b for b, e in ranges if min(e, w0) > b)
    m._flat_grad.normal_()
    flagged = torch.randperm(V, device=tr.device)[: B * T]
    tr.set_max_grad_norm(1e9)

    def flag():
        m._word_row_state.bitwise_and_(0xFE)
        m._word_row_state[flagged] |= 1
    flag()
    torch.cuda.synchronize()
    norm_us = once_us(lambda: tr._grad_clip_norm(ranges, 1.0))
    norm_bytes = 4 * dense + 4 * H * len(flagged) + V
    lines.append(f"norm, three launches on an idle device: {norm_us:8.1f} us for {norm_bytes / 1e6:.1f} MB read ({dense} dense elements in {len(ranges)} ranges, "
                 f"{len(flagged)} flagged rows of {V} x {H}, {V} state bytes) = {norm_bytes / norm_us / 1e3:.0f} GB/s")
    tr.set_max_grad_norm(None)

    def adamw():          # lr = 0, no decay: the parameters stay; zero_grad clears the gradient and the flags, so both are put back outside the timed window
        tr._adamw_ranges(ranges, 0.0, 0.0, 1, 1.0)
    got = []
    for i in range(3 + 11):
        m._flat_grad.normal_()
        flag()
        m._word_row_state.bitwise_and_(1)          # no row carries moments: the row kernel visits the flagged rows alone, like the norm
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        adamw()
        e.record()
        torch.cuda.synchronize()
        if i >= 3:
            got.append(s.elapsed_time(e) * 1e3)
    adamw_us = statistics.median(got)
    adamw_bytes = 32 * dense + 32 * H * len(flagged) + V          # p, g, m, v read; p, m, v written, g cleared
    lines.append(f"AdamW over the same ranges ({len(ranges)} dense launches + the row launch), same process: {adamw_us:8.1f} us for {adamw_bytes / 1e6:.1f} MB read + written "
                 f"= {adamw_bytes / adamw_us / 1e3:.0f} GB/s")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
