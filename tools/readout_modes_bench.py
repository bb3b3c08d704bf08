#!/usr/bin/env python3
"""What each readout mode costs at the kernel: sparch_readout_fwd_red / sparch_readout_bwd_red at the readout shapes of
cfg3 (B = 256, T = 250, 35 classes) and cfg2 (B = 128, T = 250, 20 classes) of bench.py's WORKLOADS, called the way
ReadoutLayerFn calls them under BatchNorm (folded affine in the forward, the two column sums in the backward), every mode
of functional.READOUT_MODES alternating in ONE call so that clock and thermal drift hit all of them alike.  Mode 0 goes
through the new entry points to the softmax-sum's own kernels: it is the yardstick, and the spread of its repeated runs
stands beside every ratio.

A run is LAUNCHES back-to-back launches of one kernel between two device events (the launch queue stays full: a kernel of
tens of microseconds is otherwise timed by the host's enqueue); REPS runs per (shape, direction, mode), the modes
interleaved inside each repetition.  One JSON line per (shape, direction) into profiles/readout_modes_bench.jsonl (--out):
the runs, their medians, the default's spread (max - min over median) and each mode's median over the default's.

usage: python tools/readout_modes_bench.py [--launches 2000] [--reps 7] [--out profiles/readout_modes_bench.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cfg3": dict(B=256, T=250, C=35), "cfg2": dict(B=128, T=250, C=20)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readout_modes_bench.jsonl"))
    args = ap.parse_args()
    from sparch_amd import functional as Fn
    from sparch_amd._capi import check, lib, ptr
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    dev = torch.device("cuda", 0)
    modes = list(Fn.READOUT_MODES)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    lines = []
    for name, sh in SHAPES.items():
        B, T, C = sh["B"], sh["T"], sh["C"]
        g = torch.Generator().manual_seed(1)
        rnd = lambda *s: torch.randn(*s, generator=g).to(dev)  # noqa: E731
        Wx, g_out, u0 = 1.5 * rnd(B, T, C), rnd(B, C), torch.rand(B, C, generator=g).to(dev)
        alpha = (0.83 + 0.12 * torch.rand(C, generator=g)).to(dev)
        scale, shift = (0.7 + 0.6 * torch.rand(C, generator=g)).to(dev), (0.4 * torch.rand(C, generator=g) - 0.2).to(dev)
        mean, invstd = (0.2 + 0.4 * torch.rand(C, generator=g)).to(dev), (0.5 + torch.rand(C, generator=g)).to(dev)
        out, u_save, dWx = torch.empty(B, C, device=dev), torch.empty(B, T, C, device=dev), torch.empty(B, T, C, device=dev)
        arg, ws = torch.zeros(B, C, dtype=torch.int32, device=dev), torch.empty(3, B, C, device=dev)
        stream = Fn._stream()

        def fwd(red):
            check(lib.sparch_readout_fwd_red(B, T, C, ptr(Wx), ptr(scale), ptr(shift), ptr(alpha), ptr(u0), ptr(out),
                                             ptr(u_save), red, ptr(arg), None, None, 0, stream), "sparch_readout_fwd_red")

        def bwd(red):
            check(lib.sparch_readout_bwd_red(B, T, C, ptr(g_out), ptr(Wx), ptr(mean), ptr(invstd), ptr(u_save), ptr(alpha),
                                             ptr(u0), ptr(dWx), ptr(ws), red, ptr(arg), None, None, 0, stream),
                  "sparch_readout_bwd_red")

        def run(call, red):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches):
                call(red)
            b.record()
            b.synchronize()
            return 1e3 * a.elapsed_time(b) / args.launches      # microseconds per launch

        for direction, call in (("readout_fwd", fwd), ("readout_bwd", bwd)):
            for red in range(len(modes)):                       # warm-up; the forward of a mode also leaves its arg
                fwd(red)
                for _ in range(20):
                    call(red)
            torch.cuda.synchronize()
            runs = {m: [] for m in modes}
            for _ in range(args.reps):
                for red, m in enumerate(modes):
                    if direction == "readout_bwd":
                        fwd(red)                                # (u_max: the arguments the backward reads)
                        torch.cuda.synchronize()
                    runs[m].append(run(call, red))
            Fn.check_status(dev)
            base = runs[modes[0]]
            rec = {"shape": name, **sh, "kernel": direction, "launches": args.launches, "reps": args.reps,
                   "us_per_launch": {m: [round(v, 3) for v in runs[m]] for m in modes},
                   "median_us": {m: round(med(runs[m]), 3) for m in modes},
                   "spread_of_default": round((max(base) - min(base)) / med(base), 4),
                   "ratio_to_default": {m: round(med(runs[m]) / med(base), 4) for m in modes}}
            lines.append(rec)
            print(json.dumps(rec))
    with open(args.out, "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
