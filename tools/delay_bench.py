#!/usr/bin/env python3
"""What axonal delays cost, at the cfg3 and cfg2 shapes of bench.py WORKLOADS (RadLIF [1024, 1024, 35], B = 256,
T = 250; adLIF [512, 512, 20], B = 128, T = 250; C = 700, dropout 0.1), everything in ONE call, alternating, so that
clock and thermal drift hit all arms alike:

    kernels  `sparch_delay_fwd` on the hidden layer's bf16 spike plane (B, T, H) and `sparch_delay_bwd` on its fp32
             gradient — g_x alone (fixed delays) and g_x with g_delay (learnable) — against `sparch_pack_rows` on the SAME
             tensor with full lengths: a plain row copy that reads and writes the same bytes as the gather (the delay's
             gradient reads the plane and g_y once more; its line says so in `bytes`).  Device events around ITERS
             launches, REPS times each.
    steps    one training step without the optimizer (forward, loss, backward) with delays off, fixed (all layers),
             learnable in the hidden layers' inputs only (delay_layers="hidden"), learnable in all (the first layer then
             runs the dX product it otherwise skips).  Wall clock over --steps steps, REPS times each.

max_delay = 25 steps, delays uniform in [0, 25].  The spread of the repeated runs of the reference arm (pack_rows; delays
off) stands beside every ratio — a ratio inside that spread says nothing.  One JSON line per arm into
profiles/delay_bench.jsonl (--out).

usage: python tools/delay_bench.py [--steps 10] [--iters 50] [--reps 5] [--out profiles/delay_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cfg3": dict(kind="RadLIF", sizes=[1024, 1024, 35], B=256, T=250, C=700),
          "cfg2": dict(kind="adLIF", sizes=[512, 512, 20], B=128, T=250, C=700)}
MAX_DELAY = 25
STEP_ARMS = {"off": {}, "fixed": dict(max_delay=MAX_DELAY, delay_init="uniform", learn_delays=False),
             "learn_hidden": dict(max_delay=MAX_DELAY, delay_init="uniform", delay_layers="hidden"),
             "learn_all": dict(max_delay=MAX_DELAY, delay_init="uniform")}


def med(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return round((max(v) - min(v)) / med(v), 4)


def kernel_arms(Fn, snns, sh, dev, iters, reps):
    B, T, H = sh["B"], sh["T"], sh["sizes"][0]
    g = torch.Generator().manual_seed(5)
    plane = (torch.rand(B, T, H, generator=g) < 0.1).to(torch.bfloat16).to(dev)
    grad = torch.randn(B, T, H, generator=g).to(dev)
    delay = (torch.rand(H, generator=g) * MAX_DELAY).to(dev)
    plan = snns.prepare_packing(torch.full((B,), T), B, T, dev)
    arms = {
        "pack_rows_bf16": (lambda: Fn.pack_rows(plane, plan), 2 * plane.numel() * 2),
        "delay_fwd_bf16": (lambda: Fn.delay_forward(plane, delay, MAX_DELAY), 2 * plane.numel() * 2),
        "pack_rows_f32": (lambda: Fn.pack_rows(grad, plan), 2 * grad.numel() * 4),
        "delay_bwd_gx": (lambda: Fn.delay_backward(grad, delay, MAX_DELAY, need_gdelay=False), 2 * grad.numel() * 4),
        "delay_bwd_gx_gdelay": (lambda: Fn.delay_backward(grad, delay, MAX_DELAY, x=plane),
                                3 * grad.numel() * 4 + 2 * plane.numel() * 2),
    }
    for fn, _ in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in arms}
    for _ in range(reps):
        for k, (fn, _) in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            us[k].append(1e3 * a.elapsed_time(b) / iters)
    ref = {"delay_fwd_bf16": "pack_rows_bf16", "delay_bwd_gx": "pack_rows_f32", "delay_bwd_gx_gdelay": "pack_rows_f32"}
    out = []
    for k, (_, nbytes) in arms.items():
        rec = {"what": "kernel", "arm": k, "B": B, "T": T, "K": H, "max_delay": MAX_DELAY, "iters": iters, "reps": reps,
               "bytes": nbytes, "us_per_call": [round(v, 2) for v in us[k]],
               "GBps_median": round(nbytes / med(us[k]) / 1e3, 1), "spread": spread(us[k])}
        if k in ref:
            rec["ratio_to"] = ref[k]
            rec["ratio"] = round(med(us[k]) / med(us[ref[k]]), 4)
            rec["spread_of_reference"] = spread(us[ref[k]])
        out.append(rec)
    return out


def step_arms(sparch_amd, Fn, sh, dev, steps, reps):
    B, T, C, SIZES = sh["B"], sh["T"], sh["C"], sh["sizes"]
    loss_fn = Fn.CrossEntropyLoss()
    y = torch.randint(0, SIZES[-1], (B,), generator=torch.Generator().manual_seed(2)).to(dev)
    x = (torch.rand(B, T, C, generator=torch.Generator().manual_seed(3)) < 0.05).float().to(dev)
    nets = {}
    for arm, kw in STEP_ARMS.items():
        torch.manual_seed(1)
        nets[arm] = sparch_amd.SNN((B, None, C), SIZES, neuron_type=sh["kind"], dropout=0.1, normalization="batchnorm",
                                   **kw).to(dev).train()

    def step(arm):
        net = nets[arm]
        net.zero_grad(set_to_none=True)
        out, rates = net(x)
        loss_fn(out, y).backward()

    for arm in nets:
        for _ in range(3):
            step(arm)
    Fn.check_status(dev)
    ms = {arm: [] for arm in nets}
    for _ in range(reps):
        for arm in nets:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(arm)
            torch.cuda.synchronize()
            ms[arm].append(1e3 * (time.perf_counter() - t0) / steps)
    Fn.check_status(dev)
    out = []
    for arm in nets:
        rec = {"what": "train_step", "arm": arm, **sh, "max_delay": MAX_DELAY if arm != "off" else 0, "steps": steps,
               "reps": reps, "ms_per_step": [round(v, 4) for v in ms[arm]], "spread": spread(ms[arm])}
        if arm != "off":
            rec["ratio_to_off"] = round(med(ms[arm]) / med(ms["off"]), 4)
            rec["spread_of_off"] = spread(ms["off"])
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delay_bench.jsonl"))
    args = ap.parse_args()
    import sparch_amd
    from sparch_amd import functional as Fn
    from sparch_amd import snns
    dev = torch.device("cuda", 0)
    lines = []
    for name, sh in SHAPES.items():
        for rec in kernel_arms(Fn, snns, sh, dev, args.iters, args.reps) + step_arms(sparch_amd, Fn, sh, dev, args.steps,
                                                                                  args.reps):
            rec = {"shape": name, **rec}
            lines.append(rec)
            print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
