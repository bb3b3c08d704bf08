#!/usr/bin/env python3
"""What the spike encoders cost, everything in ONE call, alternating, so that clock and thermal drift hit all arms alike:

    kernels  `sparch_spike_encode` per code (rate, if, delta) at the Speech Commands feature shape (256, 98, 40) and at
             the SHD shape (256, 250, 700), writing the bf16 plane (what `SpikeEncoder.encode` hands the network).  The
             reference arm is `sparch_expand_counts_u8` on a (B, T, K) byte tensor: a flat pass that writes the same
             plane.  Device events around ITERS launches, REPS times each.
    steps    the `bench.py --workload cfg4` train step (RadLIF [1024, 1024, 35], B = 256, one second of raw audio ->
             the HIP mel filterbank -> T = 98, C = 40; forward, loss, backward, Adam) on the dense features against the
             same step with the features encoded in front of the network (if and rate: 40 inputs; delta: 80).  Wall
             clock over --steps steps, REPS times each.

K = 40 makes layer 0 the smallest product of the step: no speed-up is expected from reading a count plane instead of
the features; the lines record what the encoder adds.  The spread of the repeated runs of the reference arm stands
beside every ratio — a ratio inside that spread says nothing.  One JSON line per arm into profiles/encode_bench.jsonl.

usage: python tools/encode_bench.py [--steps 20] [--iters 50] [--reps 5] [--out profiles/encode_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNEL_SHAPES = {"sc": (256, 98, 40), "shd": (256, 250, 700)}
CFG4 = dict(kind="RadLIF", sizes=[1024, 1024, 35], B=256, T=98, C=40, audio=16000, pdrop=0.1)
SPECS = {"rate": "rate:lo=-16,hi=8", "if": "if:gain=0.5,lo=-16,hi=8", "delta": "delta:delta=1.5"}


def med(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return round((max(v) - min(v)) / med(v), 4)


def kernel_arms(sparch_amd, Fn, name, shape, dev, iters, reps):
    B, T, K = shape
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(B, T, K, generator=g) * 24 - 16).to(dev)            # log-mel-like: [-16, 8]
    counts = (torch.rand(B, T, K, generator=g) < 0.1).to(torch.uint8).to(dev)
    encs = {code: sparch_amd.SpikeEncoder.from_spec(spec, K) for code, spec in SPECS.items()}
    arms = {"expand_counts_u8": (lambda: Fn.input_from_counts(counts), None)}
    for code, enc in encs.items():
        arms[code] = (lambda enc=enc: enc.encode(x, seed=7), enc)
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
    out = []
    for k, (_, enc) in arms.items():
        KW = K if enc is None else enc.out_features
        nbytes = B * T * (K * (1 if enc is None else 4) + (KW + 7) // 8 * 8 * 2)      # read once, the plane written once
        rec = {"what": "kernel", "shape": name, "arm": k, "B": B, "T": T, "K": K, "out_features": KW, "iters": iters,
               "reps": reps, "bytes": nbytes, "us_per_call": [round(v, 2) for v in us[k]],
               "GBps_median": round(nbytes / med(us[k]) / 1e3, 1), "spread": spread(us[k])}
        if enc is not None:
            enc.totals()
            rec["ratio_to"] = "expand_counts_u8"
            rec["ratio"] = round(med(us[k]) / med(us["expand_counts_u8"]), 4)
            rec["spread_of_reference"] = spread(us["expand_counts_u8"])
        out.append(rec)
    return out


def step_arms(sparch_amd, Fn, dev, steps, reps):
    w = CFG4
    B, C, SIZES = w["B"], w["C"], w["sizes"]
    g = torch.Generator().manual_seed(4321)
    tt = torch.arange(w["audio"]) / 16000.0
    wave = (0.1 * (torch.rand(B, w["audio"], generator=g) * 2 - 1) + 0.3 * torch.sin(2 * torch.pi * 440.0 * tt)[None]).to(dev)
    y = torch.randint(0, SIZES[-1], (B,), generator=g).to(dev)
    loss_fn = Fn.CrossEntropyLoss()
    arms = {}
    for arm in ("dense",) + tuple(SPECS):
        enc = None if arm == "dense" else sparch_amd.SpikeEncoder.from_spec(SPECS[arm], C)
        torch.manual_seed(99)
        net = sparch_amd.SNN((B, None, C if enc is None else enc.out_features), SIZES, neuron_type=w["kind"],
                             dropout=w["pdrop"], normalization="batchnorm").to(dev).train()
        arms[arm] = (net, sparch_amd.optim.Adam(net.parameters(), 1e-2), enc)

    def step(arm):
        net, opt, enc = arms[arm]
        opt.zero_grad(set_to_none=True)
        feats = Fn.fbank(wave, num_mel_bins=C)
        out, rates = net(feats if enc is None else enc.encode(feats))
        loss_fn(out, y).backward()
        opt.step()
        return rates

    density = {}
    for arm, (_, _, enc) in arms.items():
        for _ in range(5):
            rates = step(arm)
        if enc is not None:   # spikes per input feature and step over the warm-up (one read-back, outside the timing)
            density[arm] = float(enc.totals().sum()) / (5 * B * w["T"] * enc.out_features)
        density[arm + "_hidden_rate"] = float(rates.detach().mean())
    Fn.check_status(dev)
    ms = {arm: [] for arm in arms}
    for _ in range(reps):
        for arm in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(arm)
            torch.cuda.synchronize()
            ms[arm].append(1e3 * (time.perf_counter() - t0) / steps)
    Fn.check_status(dev)
    out = []
    for arm, (_, _, enc) in arms.items():
        rec = {"what": "train_step", "shape": "cfg4", "arm": arm, **w, "in_features": C if enc is None else enc.out_features,
               "steps": steps, "reps": reps, "ms_per_step": [round(v, 4) for v in ms[arm]], "spread": spread(ms[arm]),
               "hidden_rate": round(density[arm + "_hidden_rate"], 4)}
        if enc is not None:
            enc.totals()
            rec["spec"] = SPECS[arm]
            rec["input_density"] = round(density[arm], 4)
            rec["ratio_to_dense"] = round(med(ms[arm]) / med(ms["dense"]), 4)
            rec["spread_of_dense"] = spread(ms["dense"])
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_bench.jsonl"))
    args = ap.parse_args()
    import sparch_amd
    from sparch_amd import functional as Fn
    dev = torch.device("cuda", 0)
    lines = []
    for name, shape in KERNEL_SHAPES.items():
        lines += kernel_arms(sparch_amd, Fn, name, shape, dev, args.iters, args.reps)
        torch.cuda.empty_cache()
    lines += step_arms(sparch_amd, Fn, dev, args.steps, args.reps)
    for rec in lines:
        print(json.dumps(rec), flush=True)
    with open(args.out, "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
