#!/usr/bin/env python3
"""What per-row lengths cost: one training step (forward, loss, backward; no optimizer) of the cfg3 and cfg4 shapes
(bench.py WORKLOADS: RadLIF [1024, 1024, 35], B = 256, T = 250 / 98, C = 700 / 40, dropout 0.1) and of two adLIF
shapes (SHAPES below) in four modes,
alternating in ONE call so that clock and thermal drift hit all of them alike:

    a  the plain step (no lengths: the entry points without `_len`)
    b  lengths all equal to T (the `_len` kernels; the same work, plus the select)
    c  lengths uniform in [T/3, T] (the readout does less; the hidden layers run on over the padding)
    d  the lengths of (c), packed (pack=True: the `_pk` kernels on sum(lengths) rows; pack_rows / unpack_rows are timed
       with the kernels; the host-side plan, and pack_rows / unpack_rows on a hidden layer's activation, on their own)

Per kernel (functional.timer: HIP events around the cell and readout calls) and per step (wall clock over the rounds), each
mode REPS times: the spread of the repeated (a) runs stands beside every b / a ratio — a ratio inside that spread says
nothing.  One JSON line per (shape, mode) into profiles/ragged_bench.jsonl (--out).  The parent commit's library (through
SPARCH_HIP_LIB, tools/ab_libs.sh) is the yardstick for (a) itself, not this tool.

usage: python tools/ragged_bench.py [--steps 10] [--reps 3] [--out profiles/ragged_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# cfg3 / cfg4: RadLIF (the recurrent kernels).  The two adLIF shapes time the scan kernels: cfg2 (bench.py) runs them
# at one neuron per thread, adlif_wide (B H >= 524288) at four — the instantiations whose ragged box-car backward with
# the folded BatchNorm sums sits at one wave per SIMD (profiles/ragged_resources.txt).
SHAPES = {"cfg3": dict(kind="RadLIF", sizes=[1024, 1024, 35], B=256, T=250, C=700),
          "cfg4": dict(kind="RadLIF", sizes=[1024, 1024, 35], B=256, T=98, C=40),
          "cfg2": dict(kind="adLIF", sizes=[512, 512, 20], B=128, T=250, C=700),
          "adlif_wide": dict(kind="adLIF", sizes=[2048, 2048, 35], B=256, T=100, C=700)}
READOUT = ("sparch_readout_fwd", "sparch_readout_bwd")


def time_readout(Fn):
    """The readout calls carry no timer label: wrap the six entry points (plain, `_len` and `_pk` under one name)."""
    for base in READOUT:
        for name in (base, base + "_len", base + "_pk"):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_bench.jsonl"))
    args = ap.parse_args()
    import sparch_amd
    from sparch_amd import functional as Fn
    dev = torch.device("cuda", 0)
    time_readout(Fn)
    lines = []
    for name, sh in SHAPES.items():
        B, T, C, SIZES = sh["B"], sh["T"], sh["C"], sh["sizes"]
        torch.manual_seed(1)
        net = sparch_amd.SNN((B, None, C), SIZES, neuron_type=sh["kind"], dropout=0.1, normalization="batchnorm").to(dev).train()
        loss_fn = Fn.CrossEntropyLoss()
        g = torch.Generator().manual_seed(2)
        y = torch.randint(0, SIZES[-1], (B,), generator=g).to(dev)
        lens = {"a": None, "b": torch.full((B,), T), "c": torch.randint(T // 3, T + 1, (B,), generator=g)}
        lens["d"] = lens["c"]
        xs = {}
        for m, ln in lens.items():
            x = (torch.rand(B, T, C, generator=torch.Generator().manual_seed(3)) < 0.05).float()
            if ln is not None:
                x = x * (torch.arange(T)[None, :] < ln[:, None])[:, :, None]
            xs[m] = x.to(dev)

        def step(m):
            net.zero_grad(set_to_none=True)
            out, rates = net(xs[m]) if lens[m] is None else net(xs[m], lengths=lens[m], pack=(m == "d"))
            loss_fn(out, y).backward()

        for m in lens:  # warm-up: allocator pools, kernel attributes
            for _ in range(3):
                step(m)
        Fn.check_status(dev)
        runs = {m: [] for m in lens}
        for rep in range(args.reps):
            for m in lens:
                Fn.timer.reset()
                Fn.timer.enabled = True
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(m)
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) / args.steps
                tot = Fn.timer.collect()
                Fn.timer.enabled = False
                k = {n: v[1] / args.steps for n, v in tot.items()
                     if n.startswith(("rec_cell", "cell_", "readout_", "pack_rows", "unpack_rows"))}
                runs[m].append({"ms_per_step": 1e3 * wall, "kernels_ms_per_step": k})
        Fn.check_status(dev)
        kernels = sorted(runs["a"][0]["kernels_ms_per_step"])
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        of = lambda m, n: [r["kernels_ms_per_step"][n] for r in runs[m]]  # noqa: E731
        for m in lens:
            rec = {"shape": name, **sh, "mode": m, "steps": args.steps, "reps": args.reps,
                   "n_valid": B * T if lens[m] is None else int(lens[m].sum()),
                   "ms_per_step": [round(r["ms_per_step"], 4) for r in runs[m]],
                   "kernels_ms_per_step": {n: [round(v, 4) for v in of(m, n)]
                                           for n in sorted(runs[m][0]["kernels_ms_per_step"])}}
            if m != "a":
                rec["ratio_to_a"] = {n: round(med(of(m, n)) / med(of("a", n)), 4) for n in kernels}
                rec["ratio_to_a"]["step"] = round(med(rec["ms_per_step"]) / med([r["ms_per_step"] for r in runs["a"]]), 4)
            if m == "d":
                rec["ratio_to_c"] = {n: round(med(of("d", n)) / med(of("c", n)), 4) for n in kernels}
                rec["ratio_to_c"]["step"] = round(med(rec["ms_per_step"]) / med([r["ms_per_step"] for r in runs["c"]]), 4)
                from sparch_amd import snns
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(50):    # the host-side plan (sort, prefix sum, one pinned upload); the step's time holds it
                    snns.prepare_packing(lens[m], B, T, dev)
                rec["plan_host_us"] = round(1e6 * (time.perf_counter() - t0) / 50, 1)
                # the row movers on their own, at the widest hidden layer's (B, T, H) fp32 activation: HIP events around 20
                # calls each (unpack_rows does not run in a training step with a readout layer)
                plan = snns.prepare_packing(lens[m], B, T, dev)
                act = torch.rand(B, T, SIZES[0], device=dev)
                packed = Fn.pack_rows(act, plan)
                for label, call in (("pack_rows", lambda: Fn.pack_rows(act, plan)), ("unpack_rows", lambda: Fn.unpack_rows(packed, plan))):
                    call()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(20):
                        call()
                    e1.record()
                    torch.cuda.synchronize()
                    rec[label + "_hidden_ms"] = round(e0.elapsed_time(e1) / 20, 4)
            else:
                rec["spread_of_a"] = {n: round((max(of("a", n)) - min(of("a", n))) / med(of("a", n)), 4) for n in kernels}
                w = [r["ms_per_step"] for r in runs["a"]]
                rec["spread_of_a"]["step"] = round((max(w) - min(w)) / med(w), 4)
            lines.append(rec)
            print(json.dumps(rec))
        del net
    with open(args.out, "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
