#!/usr/bin/env python3
"""GPU micro-benchmark of the ITC head kernels, each alone on the chip: the rank-local pair (itc_fwd / itc_bwd, B posts) and the global-batch pair
(itc_global_fwd / _bwd on G = world * B gathered posts, B local rows), E = 512.  Method of tools/rowop_bench.py: median per-call time from HIP
events over interleaved rounds; a "call" is the launcher's whole sequence (itc_global_fwd: tile kernel + lse + loss; itc_global_bwd: strip kernel +
two small GEMMs + normalisation backward); a kernel trace of this script gives the per-kernel split.
    python tools/itc_bench.py [--rounds 15] > profiles/itc_global_bench.txt"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import smtc_amd  # noqa: F401,E402
from smtc_amd import _lib  # noqa: E402

lib = _lib.lib()
dev = torch.device("cuda:0")
st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
p = lambda t: None if t is None else C.c_void_p(t.data_ptr())


def timed(fns, rounds):
    ev = [[(torch.cuda.Event(True), torch.cuda.Event(True)) for _ in fns] for _ in range(rounds)]
    for f in fns:
        assert f() == 0 and f() == 0
    torch.cuda.synchronize()
    for r in range(rounds):
        for i, f in enumerate(fns):
            ev[r][i][0].record()
            rc = f()
            ev[r][i][1].record()
            assert rc == 0, rc
    torch.cuda.synchronize()
    out = []
    for i in range(len(fns)):
        ts = sorted(ev[r][i][0].elapsed_time(ev[r][i][1]) * 1e3 for r in range(rounds))
        out.append((ts[len(ts) // 2], ts[0], ts[-1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    a = ap.parse_args()
    E = 512
    ls = torch.full((1,), 2.6592, device=dev)
    fns, tags, keep = [], [], []
    for B in (64,):
        te, ie = torch.randn(B, E, device=dev), torch.randn(B, E, device=dev)
        tn, im, ti, ii = torch.empty_like(te), torch.empty_like(ie), torch.empty(B, device=dev), torch.empty(B, device=dev)
        lg, dl = torch.empty(B, B, device=dev), torch.randn(B, B, device=dev) / B
        dte, die, dls = torch.empty_like(te), torch.empty_like(ie), torch.zeros(1, device=dev)
        keep += [te, ie, tn, im, ti, ii, lg, dl, dte, die, dls]
        fns.append(lambda: lib.mmhip_op_itc_fwd(p(te), p(ie), p(ls), B, E, p(tn), p(im), p(ti), p(ii), p(lg), st()))
        tags.append(f"itc_fwd         B {B:4d}")
        fns.append(lambda: lib.mmhip_op_itc_bwd(p(dl), p(lg), p(tn), p(im), p(ti), p(ii), p(ls), B, E, p(dte), p(die), p(dls), st()))
        tags.append(f"itc_bwd         B {B:4d}")
    for G, Bl in ((128, 64), (512, 64), (2048, 64)):
        t, i = torch.randn(G, E, device=dev), torch.randn(G, E, device=dev)
        t, i = t / t.norm(dim=1, keepdim=True), i / i.norm(dim=1, keepdim=True)
        n = lib.mmhip_op_itc_global_ws_bytes(G, Bl)
        ws = torch.empty(n, dtype=torch.uint8, device=dev)
        rl, cl, lo = torch.empty(G, device=dev), torch.empty(G, device=dev), torch.empty(1, device=dev)
        dT, dI, dte, die = (torch.empty(Bl, E, device=dev) for _ in range(4))
        inv, dls = torch.ones(Bl, device=dev), torch.zeros(1, device=dev)
        keep += [t, i, ws, rl, cl, lo, dT, dI, dte, die, inv, dls]
        fns.append(lambda t=t, i=i, G=G, rl=rl, cl=cl, lo=lo, ws=ws, n=n: lib.mmhip_op_itc_global_fwd(p(t), p(i), p(ls), G, E, None, p(rl), p(cl), p(lo), p(ws), n, st()))
        tags.append(f"itc_global_fwd  G {G:4d} B_local {Bl}")
        fns.append(lambda t=t, i=i, G=G, Bl=Bl, rl=rl, cl=cl, ws=ws, n=n, dT=dT, dI=dI, dte=dte, die=die, inv=inv, dls=dls:
                   lib.mmhip_op_itc_global_bwd(p(t), p(i), p(ls), p(rl), p(cl), G, Bl, G - Bl, E, 1.0, p(dT), p(dI), p(dls), p(inv), p(inv), p(dte), p(die), p(ws), n, st()))
        tags.append(f"itc_global_bwd  G {G:4d} B_local {Bl}")
    print(f"# rounds={a.rounds}; us = median (min .. max) per call, alone on the chip, E = {E}, fp32")
    for tag, (med, lo_, hi) in zip(tags, timed(fns, a.rounds)):
        print(f"{tag:40s} {med:8.1f} us  ({lo_:.1f} .. {hi:.1f})")


if __name__ == "__main__":
    main()
