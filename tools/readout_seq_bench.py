#!/usr/bin/env python3
"""What a per-step readout costs: one training step (forward, loss, backward; no optimizer) of the cfg3 and cfg2 shapes
(bench.py WORKLOADS: RadLIF [1024, 1024, 35], B = 256, T = 250, C = 700 and adLIF [512, 512, 20], B = 128, T = 250,
C = 700; dropout 0.1) in three modes, alternating in ONE call so that clock and thermal drift hit all of them alike:

    a  the plain step: net(x), cross-entropy on out
    b  net(x, per_step="sum"), cross-entropy on out plus 0.5 x exp.per_step_nll on the running sum from step 10 on (what
       SPARCH_PER_STEP_LOSS=0.5:10 trains with): the `_seq` readout kernels, and the loss's own torch kernels
    c  for scale, the only route there was: the same loss from StreamingSNN(fused=True) one-step outputs, T calls of
       step() per "step" — FORWARD ONLY, in eval mode, without gradients

Per kernel (functional.timer: HIP events around the cell and readout calls) and per step (wall clock over the rounds), each
mode REPS times.  No target for b / a: the plain readout kernels are tens of microseconds of a step of milliseconds, so the
ratio stands beside the spread of the repeated (a) runs and the record says whether it is outside it.  One JSON line per
(shape, mode) into profiles/readout_seq_bench.jsonl (--out).

usage: python tools/readout_seq_bench.py [--steps 10] [--reps 3] [--out profiles/readout_seq_bench.jsonl]
"""
import argparse
import copy
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cfg3": dict(kind="RadLIF", sizes=[1024, 1024, 35], B=256, T=250, C=700),
          "cfg2": dict(kind="adLIF", sizes=[512, 512, 20], B=128, T=250, C=700)}
READOUT = ("sparch_readout_fwd", "sparch_readout_bwd")
W, T0 = 0.5, 10


def time_readout(Fn):
    """The readout calls carry no timer label: wrap the entry points (plain and `_seq` under one name)."""
    for base in READOUT:
        for name in (base, base + "_seq"):
            def timed(*a, _f=getattr(Fn.lib, name), _label=base.replace("sparch_", "")):
                tok = Fn.timer.start(_label)
                rc = _f(*a)
                Fn.timer.stop(tok)
                return rc
            setattr(Fn.lib, name, timed)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "readout_seq_bench.jsonl"))
    args = ap.parse_args()
    import sparch_amd
    from sparch_amd import exp
    from sparch_amd import functional as Fn
    dev = torch.device("cuda", 0)
    time_readout(Fn)
    lines = []
    for name, sh in SHAPES.items():
        B, T, C, SIZES = sh["B"], sh["T"], sh["C"], sh["sizes"]
        torch.manual_seed(1)
        net = sparch_amd.SNN((B, None, C), SIZES, neuron_type=sh["kind"], dropout=0.1, normalization="batchnorm").to(dev).train()
        stream = sparch_amd.StreamingSNN(copy.deepcopy(net).eval(), B, fused=True)
        loss_fn = Fn.CrossEntropyLoss()
        g = torch.Generator().manual_seed(2)
        y = torch.randint(0, SIZES[-1], (B,), generator=g).to(dev)
        x = (torch.rand(B, T, C, generator=torch.Generator().manual_seed(3)) < 0.05).float().to(dev)
        seq_buf = torch.empty(B, T, SIZES[-1], device=dev)

        def step(m):
            if m == "c":
                with torch.no_grad():
                    stream.reset()
                    for t in range(T):
                        seq_buf[:, t] = stream.step(x[:, t:t + 1])
                    return loss_fn(seq_buf[:, -1], y) + W * exp.per_step_nll(seq_buf, y, None, T0)
            net.zero_grad(set_to_none=True)
            if m == "a":
                out, rates = net(x)
                loss = loss_fn(out, y)
            else:
                out, rates, seq = net(x, per_step="sum")
                loss = loss_fn(out, y) + W * exp.per_step_nll(seq, y, None, T0)
            loss.backward()
            return loss

        modes = ("a", "b", "c")
        for m in modes:  # warm-up: allocator pools, kernel attributes
            for _ in range(3 if m != "c" else 1):
                step(m)
        Fn.check_status(dev)
        runs = {m: [] for m in modes}
        for rep in range(args.reps):
            for m in modes:
                Fn.timer.reset()
                Fn.timer.enabled = m != "c"
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(m)
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) / args.steps
                tot = Fn.timer.collect() if m != "c" else {}
                Fn.timer.enabled = False
                k = {n: v[1] / args.steps for n, v in tot.items() if n.startswith(("rec_cell", "cell_", "readout_"))}
                runs[m].append({"ms_per_step": 1e3 * wall, "kernels_ms_per_step": k})
        Fn.check_status(dev)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        of = lambda m, n: [r["kernels_ms_per_step"][n] for r in runs[m]]  # noqa: E731
        wall_a = [r["ms_per_step"] for r in runs["a"]]
        spread = (max(wall_a) - min(wall_a)) / med(wall_a)
        for m in modes:
            rec = {"shape": name, **sh, "mode": m, "steps": args.steps, "reps": args.reps,
                   "ms_per_step": [round(r["ms_per_step"], 4) for r in runs[m]],
                   "kernels_ms_per_step": {n: [round(v, 4) for v in of(m, n)] for n in sorted(runs[m][0]["kernels_ms_per_step"])}}
            if m == "a":
                rec["spread_of_a"] = {n: round((max(of("a", n)) - min(of("a", n))) / med(of("a", n)), 4)
                                      for n in sorted(runs["a"][0]["kernels_ms_per_step"])}
                rec["spread_of_a"]["step"] = round(spread, 4)
            else:
                ratio = med(rec["ms_per_step"]) / med(wall_a)
                rec["ratio_to_a"] = {"step": round(ratio, 4)}
                if m == "b":
                    rec["ratio_to_a"].update({n: round(med(of("b", n)) / med(of("a", n)), 4) for n in ("readout_fwd", "readout_bwd")})
                    rec["step_ratio_outside_spread_of_a"] = bool(abs(ratio - 1.0) > spread)
                else:
                    rec["note"] = "forward only, eval mode, no gradients: T one-step StreamingSNN calls per step"
                    rec["us_per_stream_step"] = round(1e3 * med(rec["ms_per_step"]) / T, 2)
            lines.append(rec)
            print(json.dumps(rec))
        del net, stream
    with open(args.out, "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
