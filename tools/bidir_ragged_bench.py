#!/usr/bin/env python3
"""What lengths cost a bidirectional network: one training step (forward, loss, backward; no optimizer) of two HD-like
shapes (B = 256, T = 98, C = 40, 20 classes, dropout 0.1, BatchNorm: tools/ragged_bench.py's cfg4 input) — adLIF 3 x 512 and
RadLIF 3 x 1024, bidirectional — in three modes, alternating in ONE call so that clock and thermal drift hit all of them
alike (tools/ragged_bench.py's protocol):

    a  today's padded bidirectional step, no lengths (the two-direction entry points; the reverse direction starts on
       the padding)
    b  lengths uniform in [T/3, T] (ragged_bench.py's distribution), masked: bidir_split -> the one-direction `_len`
       kernels on 2B rows -> bidir_join, and their adjoints
    c  the same lengths, pack=True: the `_pk` kernels on 2 sum(lengths) rows

Per kernel (functional.timer: HIP events around the cell, readout and bidir_* calls) and per step (wall clock), each mode
REPS times: the spread of the repeated (a) runs stands beside every ratio — a ratio inside that spread says nothing.  Per
layer, the launches and bytes the four movers add (computed from the shapes: what each kernel reads and writes once).
One JSON line per (shape, mode) into profiles/bidir_ragged_bench.jsonl (--out).

usage: python tools/bidir_ragged_bench.py [--steps 10] [--reps 3] [--out profiles/bidir_ragged_bench.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"adlif_3x512": dict(kind="adLIF", sizes=[512, 512, 20], B=256, T=98, C=40),
          "radlif_3x1024": dict(kind="RadLIF", sizes=[1024, 1024, 20], B=256, T=98, C=40)}
READOUT = ("sparch_readout_fwd", "sparch_readout_bwd")
TIMED = ("rec_cell", "cell_", "readout_", "pack_rows", "unpack_rows", "bidir_")


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


def mover_bytes(B, T, H, n, packed):
    """Bytes each of a layer's four movers reads + writes once (H units per direction, n = sum(lengths) valid steps): the
    split of the fp32 drive and its adjoint, the join of the bf16 plane (between layers only the plane travels) and its
    adjoint on the fp32 gradient.  Masked tensors are written whole (zero tails), packed ones have no tails."""
    one, two = (n, 2 * n) if packed else (B * T, 2 * B * T)
    return {"bidir_split": 4 * H * (n + two), "bidir_split_bwd": 4 * H * (2 * n + one),
            "bidir_join": 2 * H * (2 * n) + 2 * (2 * H) * one, "bidir_join_bwd": 4 * (2 * H) * n + 4 * H * two}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bidir_ragged_bench.jsonl"))
    args = ap.parse_args()
    import sparch_amd
    from sparch_amd import functional as Fn
    dev = torch.device("cuda", 0)
    time_readout(Fn)
    lines = []
    for name, sh in SHAPES.items():
        B, T, C, SIZES = sh["B"], sh["T"], sh["C"], sh["sizes"]
        torch.manual_seed(1)
        net = sparch_amd.SNN((B, None, C), SIZES, neuron_type=sh["kind"], dropout=0.1, normalization="batchnorm",
                             bidirectional=True).to(dev).train()
        loss_fn = Fn.CrossEntropyLoss()
        g = torch.Generator().manual_seed(2)
        y = torch.randint(0, SIZES[-1], (B,), generator=g).to(dev)
        ragged = torch.randint(T // 3, T + 1, (B,), generator=g)
        lens = {"a": None, "b": ragged, "c": ragged}
        x = (torch.rand(B, T, C, generator=torch.Generator().manual_seed(3)) < 0.05).float()
        x = (x * (torch.arange(T)[None, :] < ragged[:, None])[:, :, None]).to(dev)   # (the same padded batch for all modes)

        def step(m):
            net.zero_grad(set_to_none=True)
            out, rates = net(x) if lens[m] is None else net(x, lengths=lens[m], pack=(m == "c"))
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
                k = {n_: v[1] / args.steps for n_, v in tot.items() if n_.startswith(TIMED)}
                calls = {n_: v[0] / args.steps for n_, v in tot.items() if n_.startswith("bidir_")}
                runs[m].append({"ms_per_step": 1e3 * wall, "kernels_ms_per_step": k, "calls": calls})
        Fn.check_status(dev)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        wall = lambda m: [r["ms_per_step"] for r in runs[m]]  # noqa: E731
        n_valid = int(ragged.sum())
        for m in lens:
            names = sorted(runs[m][0]["kernels_ms_per_step"])
            rec = {"shape": name, **sh, "bidirectional": True, "mode": m, "steps": args.steps, "reps": args.reps,
                   "n_valid": B * T if lens[m] is None else n_valid,
                   "ms_per_step": [round(v, 4) for v in wall(m)],
                   "kernels_ms_per_step": {n_: [round(r["kernels_ms_per_step"][n_], 4) for r in runs[m]] for n_ in names}}
            if m == "a":
                w = wall("a")
                rec["spread_of_a"] = {"step": round((max(w) - min(w)) / med(w), 4)}
            else:
                rec["ratio_to_a"] = {"step": round(med(wall(m)) / med(wall("a")), 4)}
                rec["mover_launches_per_layer_and_step"] = {n_: round(c / 2, 2) for n_, c in runs[m][0]["calls"].items()}
                rec["mover_bytes_per_layer"] = mover_bytes(B, T, SIZES[0], n_valid, m == "c")
                rec["mover_ms_per_step"] = round(sum(med([r["kernels_ms_per_step"][n_] for r in runs[m]])
                                                     for n_ in names if n_.startswith("bidir_")), 4)
            lines.append(rec)
            print(json.dumps(rec))
        del net
    with open(args.out, "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
