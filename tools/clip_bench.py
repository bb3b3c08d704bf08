#!/usr/bin/env python3
"""What gradient clipping inside the optimizer step costs: one training step INCLUDING the optimizer (zero_grad, forward,
loss, backward, step; eager launches) of the cfg2 and cfg3 shapes (bench.py WORKLOADS: adLIF [512, 512, 20], B = 128 —
host-bound, launches matter — and RadLIF [1024, 1024, 35], B = 256; T = 250, C = 700, dropout 0.1) in four modes,
alternating in ONE call so that clock and thermal drift hit all of them alike:

    a  optim.Adam()                                   no clipping: the C calls of every earlier version
    b  optim.Adam(max_grad_norm=inf)                  the norm is taken, nothing is scaled (coefficient 1)
    c  optim.Adam(max_grad_norm=1e-6)                 every step clips
    d  torch.nn.utils.clip_grad_norm_(params, 1.0) in front of the plain step (a)

Per step (wall clock over `--steps` steps), each mode `--reps` times: the spread of the repeated (a) runs stands beside
every ratio to (a) — a ratio inside that spread says nothing.  One JSON line per (shape, mode) into
profiles/clip_bench.jsonl (--out).  Each mode has its own optimizer (its own moments) on the one network.

The kernels' own times come from a profiler, not from this process: run
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/clip_bench.py --shapes cfg3 --modes c \\
        --reps 1 --out /dev/null
and append the optimizer's rows of DIR/**/*kernel_stats.csv with
    python tools/clip_bench.py --merge-kernel-stats that.csv --shapes cfg3 [--out profiles/clip_bench.jsonl]

usage: python tools/clip_bench.py [--steps 10] [--reps 3] [--shapes cfg2,cfg3] [--modes a,b,c,d] [--out FILE]
"""
import argparse
import csv
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cfg2": dict(kind="adLIF", sizes=[512, 512, 20], B=128, T=250, C=700),
          "cfg3": dict(kind="RadLIF", sizes=[1024, 1024, 35], B=256, T=250, C=700)}
KERNELS = ("grad_sumsq_kernel", "clip_finish_kernel", "adam_clip_kernel", "adam_kernel", "scale_grads_kernel")


def merge_kernel_stats(path, shape, out):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = next((k for k in KERNELS if k in r.get("Name", "")), None)
            if name:
                rows.append({"kernel": name, "calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 3),
                             "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3)})
    rec = {"shape": shape, "mode": "kernel_stats", "source": "rocprofv3 --kernel-trace --stats, mode c", "kernels": rows}
    print(json.dumps(rec))
    with open(out, "a") as f:
        f.write(json.dumps(rec) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="cfg2,cfg3")
    ap.add_argument("--modes", default="a,b,c,d")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_bench.jsonl"))
    ap.add_argument("--merge-kernel-stats", default=None)
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.shapes, args.out)
    import sparch_amd
    from sparch_amd import functional as Fn
    from sparch_amd.optim import Adam
    dev = torch.device("cuda", 0)
    modes = args.modes.split(",")
    lines = []
    for name in args.shapes.split(","):
        sh = SHAPES[name]
        B, T, C, SIZES = sh["B"], sh["T"], sh["C"], sh["sizes"]
        torch.manual_seed(1)
        net = sparch_amd.SNN((B, None, C), SIZES, neuron_type=sh["kind"], dropout=0.1, normalization="batchnorm").to(dev).train()
        loss_fn = Fn.CrossEntropyLoss()
        g = torch.Generator().manual_seed(2)
        y = torch.randint(0, SIZES[-1], (B,), generator=g).to(dev)
        x = (torch.rand(B, T, C, generator=g) < 0.05).float().to(dev)
        params = list(net.parameters())
        opts = {"a": Adam(params, 1e-3), "b": Adam(params, 1e-3, max_grad_norm=float("inf")),
                "c": Adam(params, 1e-3, max_grad_norm=1e-6), "d": Adam(params, 1e-3)}

        def step(m):
            opts[m].zero_grad(set_to_none=True)
            out, _ = net(x)
            loss_fn(out, y).backward()
            if m == "d":
                torch.nn.utils.clip_grad_norm_(params, 1.0)
            opts[m].step()

        for m in modes:  # warm-up: allocator pools, kernel attributes
            for _ in range(3):
                step(m)
        Fn.check_status(dev)
        runs = {m: [] for m in modes}
        for rep in range(args.reps):
            for m in modes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(m)
                torch.cuda.synchronize()
                runs[m].append(1e3 * (time.perf_counter() - t0) / args.steps)
        Fn.check_status(dev)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        for m in modes:
            rec = {"shape": name, **sh, "mode": m, "steps": args.steps, "reps": args.reps,
                   "n_params": sum(p.numel() for p in params), "n_tensors": len(params),
                   "ms_per_step": [round(v, 4) for v in runs[m]], "median_ms_per_step": round(med(runs[m]), 4)}
            if m in ("b", "c"):
                s = opts[m].clip_stats()
                rec["clip_stats"] = {k: s[k] for k in ("steps", "clipped", "skipped")}
            if "a" in runs:
                if m == "a":
                    rec["spread_of_a"] = round((max(runs["a"]) - min(runs["a"])) / med(runs["a"]), 4)
                else:
                    rec["ratio_to_a"] = round(med(runs[m]) / med(runs["a"]), 4)
            lines.append(rec)
            print(json.dumps(rec))
        del net, opts
    if args.out != "/dev/null":
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
