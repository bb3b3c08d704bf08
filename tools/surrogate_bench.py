#!/usr/bin/env python3
"""Per-launch time of the spiking backward kernels under each surrogate gradient, against the box-car of the same
build, alternating: `cell_bwd[adLIF]` (scan kernel) and `rec_cell_bwd[RadLIF]` (persistent kernel) as the KernelTimer
labels report them, at the headline shape (B 256, T 250, H 1024) and at B 128, T 250, H 512.

    python tools/surrogate_bench.py [--rounds R] [--iters N] [--out profiles/surrogate_bench.json]

A round runs the four surrogates one after another, N forward + backward passes each (HIP events around the C-ABI
call); the figure of a surrogate is the median over the rounds of its per-launch mean, the spread is min .. max over the
rounds.  The first round is a warm-up and is dropped.  Needs an MI355X; prints the JSON it writes."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from sparch_amd import functional as Fn  # noqa: E402
from sparch_amd.snns import SURROGATE_DEFAULT_SCALE  # noqa: E402

SHAPES = {"headline": (256, 250, 1024), "3x512": (128, 250, 512)}
KINDS = {"adLIF": "cell_bwd[adLIF]", "RadLIF": "rec_cell_bwd[RadLIF]"}


def inputs(kind, B, T, H, dev):
    g = torch.Generator().manual_seed(0)
    V = torch.nn.init.orthogonal_(torch.empty(H, H), generator=g).to(dev) if kind == "RadLIF" else None
    Wx = (torch.randn(B, T, H, generator=g) * 1.2 + 0.2).to(dev).requires_grad_(True)
    p = dict(alpha=torch.rand(H, generator=g) * 0.14 + 0.82, beta=torch.rand(H, generator=g) * 0.024 + 0.967,
             a=torch.rand(H, generator=g) * 2 - 1, b=torch.rand(H, generator=g) * 2)
    p = {k: v.to(dev) for k, v in p.items()}
    states = [torch.rand(B, H, generator=g).to(dev) for _ in range(3)]
    return Wx, p, V, states, torch.randn(B, T, H, generator=g).to(dev)


def one_block(kind, label, data, surrogate, iters):
    Wx, p, V, (u0, w0, s0), gs = data
    Fn.timer.collect()
    Fn.timer.reset()
    for _ in range(iters):
        s = Fn.SpikingCellFn.apply(kind, 1.0, Wx, p["alpha"], p["beta"], p["a"], p["b"], V, u0, w0, s0, None, surrogate)
        (s * gs).sum().backward()
        Wx.grad = None
    n, ms = Fn.timer.collect()[label]
    assert n == iters
    return ms / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="profiles/surrogate_bench.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    Fn.timer.enabled = True
    forms = [None] + [(n, k) for n, k in SURROGATE_DEFAULT_SCALE.items() if k is not None]
    result = {"unit": "ms per launch", "rounds": a.rounds, "iters_per_round": a.iters,
              "figure": "median over rounds of the per-launch mean; spread = min .. max over rounds; first round dropped"}
    for shape, (B, T, H) in SHAPES.items():
        for kind, label in KINDS.items():
            data = inputs(kind, B, T, H, "cuda")
            runs = {("boxcar" if f is None else f[0]): [] for f in forms}
            for r in range(a.rounds + 1):
                for f in forms:
                    t = one_block(kind, label, data, f, a.iters)
                    if r:
                        runs["boxcar" if f is None else f[0]].append(t)
            Fn.check_status()
            base = statistics.median(runs["boxcar"])
            result[f"{label} {shape} B{B} T{T} H{H}"] = {
                n: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                    "vs_boxcar": round(statistics.median(v) / base, 4)} for n, v in runs.items()}
            del data
            torch.cuda.empty_cache()
    text = json.dumps(result, indent=1)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
