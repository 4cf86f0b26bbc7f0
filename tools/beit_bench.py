#!/usr/bin/env python3
"""The late-fusion train step (smtc_amd.mm_late.MMLate_Model.train_step) with the BEiT image tower beside the same step with ViT, at the config-2
shape (Bernice + a B/16 image tower, B = 64, T = 128, bf16, attention fusion, no auxiliary loss), in ONE process on one box:

  * the ViT step twice, before and after the BEiT steps: the difference of the two runs is the run-to-run spread the comparison has to be read against;
  * the BEiT step at drop_path_rate 0 (the fused residual epilogues, as ViT) and at 0.1 (the reference's training: 22 of the 24 residual GEMMs write
    their branch to scratch and a second launch adds it per post), each with the image tower's span (mmhip_step_spans: fork -> tower end, median);
    the difference of the two spans is what the drop-path adds cost;
  * the attention forward of one tower layer (64 posts x 12 heads x 197 tokens) per launch with and without the relative position bias, HIP events
    around REPS launches enqueued back to back on an idle device.

Prints and writes profiles/beit_bench.txt.

    python tools/beit_bench.py [--steps 20] [--warmup 5] [--layers 12]
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

REPS = 10


def step_and_tower(img, rate, B, T, layers, steps, warmup):
    """-> (ms/step, image tower span in ms) of one freshly built model"""
    from smtc_amd.mm_late import MMLate_Model
    cfg = types.SimpleNamespace(batch_size=B, num_labels=3, use_clip_loss=False, beta_itc=None, use_tim_loss=False, beta_itm=None, max_length=T, dropout=0.05)
    arch = dict(layers_txt=layers, layers_img=layers)
    if img == "beit":
        arch["drop_path_rate"] = rate
    tr = MMLate_Model(cfg, "bernice", img, "attention", dtype="bf16", seed=0, arch=arch)
    m, lib = tr.model, _lib.lib()
    a = m.arch
    ids, mask, pixels, onehot = synthetic_batch(a["vocab"], 3, B, T, 1, a["txt_kind"], a["pad_id"], False, a["image"], tr.device)
    n = [0]

    def one():
        n[0] += 1
        tr.train_step(ids, mask, pixels, onehot, None, 1e-5, 0.00025, n[0])
    ms = timed(one, steps, warmup)
    rows = []
    _lib.check(lib.mmhip_step_spans(m._handle, 1, None))
    for _ in range(8):
        one()
        buf = (ctypes.c_float * 5)()
        _lib.check(lib.mmhip_step_spans(m._handle, 1, buf))
        rows.append(list(buf))
    _lib.check(lib.mmhip_step_spans(m._handle, 0, None))
    del tr
    torch.cuda.empty_cache()
    return ms, statistics.median(r[0] for r in rows[1:])


def attention_us(B, S=197, heads=12):
    """-> (us per launch without bias, with bias) of the bf16 attention forward of one image layer"""
    lib, s, dev = _lib.lib(), _lib.stream_ptr(), "cuda:0"
    H, ld = heads * 64, (S + 3) // 4 * 4
    qkv = torch.randn(B * S, 3 * H, device=dev).to(torch.bfloat16)
    ctx = torch.empty(B * S, H, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B, heads, S, device=dev)
    bias = torch.zeros(heads, S, ld, device=dev)
    bias[:, :, :S] = torch.randn(heads, S, S, device=dev)
    P = _lib.ptr

    def plain():
        for _ in range(REPS):
            _lib.check(lib.mmhip_op_attn_fwd(_lib.BF16, P(qkv), None, P(ctx), P(lse), B, S, heads, 0.0, 0, 0, s), "attn_fwd")

    def biased():
        for _ in range(REPS):
            _lib.check(lib.mmhip_op_attn_fwd_bias(_lib.BF16, P(qkv), P(bias), ld, P(ctx), P(lse), B, S, heads, s), "attn_fwd_bias")
    return once_us(plain) / REPS, once_us(biased) / REPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beit_bench.txt"))
    args = ap.parse_args()
    B, T, L = args.batch, 128, args.layers
    lines = [f"late-fusion train step, config-2 shape (Bernice + B/16 image tower, {L} + {L} layers), B = {B}, T = {T}, bf16, attention fusion, no auxiliary "
             f"loss; {torch.cuda.get_device_name(0)}"]
    runs = [("vit", 0.0, "vit (first run)"), ("beit", 0.0, "beit, drop_path_rate 0"), ("beit", 0.1, "beit, drop_path_rate 0.1"), ("vit", 0.0, "vit (second run)")]
    res = []
    for img, rate, label in runs:
        ms, tower = step_and_tower(img, rate, B, T, L, args.steps, args.warmup)
        res.append((ms, tower))
        lines.append(f"{label:26s} {ms:8.3f} ms/step {B / ms * 1e3:9.1f} posts/s   image tower span {tower:7.3f} ms")
    vit_ms, vit_tower = 0.5 * (res[0][0] + res[3][0]), 0.5 * (res[0][1] + res[3][1])
    lines.append(f"run-to-run spread of the vit step: {abs(res[0][0] - res[3][0]):6.3f} ms (tower span: {abs(res[0][1] - res[3][1]):6.3f} ms)")
    lines.append(f"beit at rate 0 minus the vit mean: step {res[1][0] - vit_ms:+7.3f} ms, tower span {res[1][1] - vit_tower:+7.3f} ms "
                 f"(relative position bias in {L} attention launches, mean-pool pooler, no final LayerNorm over the tokens)")
    adds = res[2][1] - res[1][1]
    lines.append(f"drop path: beit at rate 0.1 minus rate 0: step {res[2][0] - res[1][0]:+7.3f} ms, tower span {adds:+7.3f} ms = {100 * adds / res[2][1]:5.1f} % of the "
                 f"tower's span ({2 * max(L - 1, 0)} branches through scratch + a per-post add each)")
    plain, biased = attention_us(B)
    lines.append(f"attention forward of one image layer ({B} posts x 12 heads x 197 tokens, bf16), per launch, {REPS} launches back to back on an idle device: "
                 f"without bias {plain:7.1f} us, with bias {biased:7.1f} us ({100 * (biased - plain) / plain:+5.1f} %)")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
