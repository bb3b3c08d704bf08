#!/usr/bin/env python3
"""What synaptic currents cost ("Synaptic currents"), everything in ONE call, alternating, so that
clock and thermal drift hit all arms alike:

    kernels  `sparch_synapse_fwd` and `sparch_synapse_bwd` (g_z alone: a fixed synapse; g_z with g_gamma: a learnable
             one; with BatchNorm's column sums folded in) on a layer's (B, T, H) drive at B = 256, T = 250, H = 1024
             (cfg3) and H = 512 (cfg2), and beside them the LIF scan on the SAME tensors — `cell_fwd[LIF]` without the fp32 spike tensor, `cell_bwd[LIF]` — as the
             yardstick of what a time scan reaches on this part.  Every line carries the bytes its kernel has to move
             and bytes / time; nothing here says what fraction of the HBM bandwidth that is.  Device events around ITERS
             launches, REPS times each.
    steps    one training step without the optimizer (forward, loss, backward) at the cfg3 and cfg2 shapes of bench.py
             WORKLOADS (RadLIF [1024, 1024, 35], B = 256; adLIF [512, 512, 20], B = 128; T = 250, C = 700, dropout 0.1)
             with the synapse off, fixed and learnable on every hidden layer.  Wall clock over --steps steps, REPS times.

The spread of the repeated runs of the reference arm stands beside every ratio — a ratio inside that spread says
nothing.  One JSON line per arm into profiles/synapse_bench.jsonl (--out).

usage: python tools/synapse_bench.py [--steps 10] [--iters 50] [--reps 5] [--out profiles/synapse_bench.jsonl]
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
KERNEL_B = 256
LIMITS = (0.0, 0.9)
STEP_ARMS = {"off": {}, "fixed": dict(synapse=LIMITS, learn_synapse=False), "learn": dict(synapse=LIMITS)}


def med(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return round((max(v) - min(v)) / med(v), 4)


def kernel_arms(Fn, sh, dev, iters, reps):
    B, T, H = KERNEL_B, sh["T"], sh["sizes"][0]
    g = torch.Generator().manual_seed(5)
    Wx = torch.randn(B, T, H, generator=g).to(dev)
    grad = torch.randn(B, T, H, generator=g).to(dev)
    gamma = (torch.rand(H, generator=g) * 0.9).to(dev)
    alpha = (torch.rand(H, generator=g) * 0.1 + 0.85).to(dev)
    u0, s0 = torch.rand(B, H, generator=g).to(dev), torch.rand(B, H, generator=g).to(dev)
    mean, invstd = torch.randn(H, generator=g).to(dev), (torch.rand(H, generator=g) + 0.5).to(dev)
    cur = Fn.synapse_forward(Wx, gamma, LIMITS)
    cell_kw = dict(B=B, dirs=1, theta=1.0, p_drop=0.0, seed=0)
    _, _, saved, _ = Fn.cell_forward("LIF", Wx, None, None, {"alpha": alpha}, u0, None, s0, want_s_out=False, **cell_kw)
    n = Wx.numel()
    arms = {
        "cell_fwd_LIF": (lambda: Fn.cell_forward("LIF", Wx, None, None, {"alpha": alpha}, u0, None, s0, want_s_out=False,
                                                 **cell_kw), 10 * n),     # reads Wx; writes the bf16 plane and u
        "synapse_fwd": (lambda: Fn.synapse_forward(Wx, gamma, LIMITS), 8 * n),
        "cell_bwd_LIF": (lambda: Fn.cell_backward("LIF", grad, None, {"alpha": alpha}, u0, None, s0, saved, T=T, H=H,
                                                  **cell_kw), 12 * n),    # reads g and u; writes dWx
        "synapse_bwd_gz": (lambda: Fn.synapse_backward(grad, None, gamma, LIMITS, need_ggamma=False), 8 * n),
        "synapse_bwd_gz_ggamma": (lambda: Fn.synapse_backward(grad, cur, gamma, LIMITS), 12 * n),
        # under BatchNorm: the projection is read too, for the normalisation's column sums (the LIF backward folds them
        # in likewise; its line here runs without them)
        "synapse_bwd_gz_ggamma_bn": (lambda: Fn.synapse_backward(grad, cur, gamma, LIMITS, bn=(Wx, mean, invstd)), 16 * n),
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
    ref = {"synapse_fwd": "cell_fwd_LIF", "synapse_bwd_gz": "cell_bwd_LIF", "synapse_bwd_gz_ggamma": "cell_bwd_LIF",
           "synapse_bwd_gz_ggamma_bn": "cell_bwd_LIF"}
    out = []
    for k, (_, nbytes) in arms.items():
        rec = {"what": "kernel", "arm": k, "B": B, "T": T, "H": H, "iters": iters, "reps": reps, "bytes": nbytes,
               "us_per_call": [round(v, 2) for v in us[k]], "GBps_median": round(nbytes / med(us[k]) / 1e3, 1),
               "spread": spread(us[k])}
        if k in ref:
            rec["yardstick"] = ref[k]
            rec["GBps_ratio_to_yardstick"] = round((nbytes / med(us[k])) / (arms[ref[k]][1] / med(us[ref[k]])), 4)
            rec["spread_of_yardstick"] = spread(us[ref[k]])
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
        rec = {"what": "train_step", "arm": arm, **sh, "limits": list(LIMITS) if arm != "off" else None, "steps": steps,
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synapse_bench.jsonl"))
    args = ap.parse_args()
    import sparch_amd
    from sparch_amd import functional as Fn
    dev = torch.device("cuda", 0)
    lines = []
    for name, sh in SHAPES.items():
        for rec in kernel_arms(Fn, sh, dev, args.iters, args.reps) + step_arms(sparch_amd, Fn, sh, dev, args.steps,
                                                                             args.reps):
            rec = {"shape": name, **rec}
            lines.append(rec)
            print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
