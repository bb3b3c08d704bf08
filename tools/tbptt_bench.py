#!/usr/bin/env python3
"""What chunking a training step costs: one training step (forward, loss, backward; no optimizer) of the cfg3 and cfg2
shapes (bench.py WORKLOADS: RadLIF [1024, 1024, 35], B = 256, T = 250; adLIF [512, 512, 20], B = 128, T = 250; C = 700,
dropout 0.1) and of a wide adLIF shape (four neurons per thread in the scan kernels) in four modes, alternating in ONE
call so that clock and thermal drift hit all of them alike:

    a  today's whole-sequence call (the entry points without `_st`)
    b  the stateful call with one chunk: a `state` that requires its gradient given, the final state returned and in the
       loss — every layer's backward is the `_st` kernel, all six (B, H) state gradients per layer are moved
    c  5 chunks of T / 5 steps chained with the states kept in the graph: one backward through all of them (exact; the
       `_st` kernels in every chunk)
    d  the same 5 chunks, each started from the detached state and backpropagated on its own (truncated BPTT: no
       gradient arrives on a state or leaves through one, so the hidden layers issue the PLAIN backward kernels — what
       SPARCH_TBPTT runs)

Per step (wall clock over the rounds), each mode REPS times: the spread of the repeated (a) runs stands beside every
ratio — a ratio inside that spread says nothing.  One JSON line per (shape, mode) into profiles/tbptt_bench.jsonl
(--out).

usage: python tools/tbptt_bench.py [--steps 10] [--reps 3] [--out profiles/tbptt_bench.jsonl]
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
          "cfg2": dict(kind="adLIF", sizes=[512, 512, 20], B=128, T=250, C=700),
          "adlif_wide": dict(kind="adLIF", sizes=[2048, 2048, 35], B=256, T=100, C=700)}
CHUNKS = 5
MODES = ("a", "b", "c", "d")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tbptt_bench.jsonl"))
    args = ap.parse_args()
    import sparch_amd
    from sparch_amd import functional as Fn
    from sparch_amd.snns import detach_state
    dev = torch.device("cuda", 0)
    lines = []
    for name, sh in SHAPES.items():
        B, T, C, SIZES = sh["B"], sh["T"], sh["C"], sh["sizes"]
        torch.manual_seed(1)
        net = sparch_amd.SNN((B, None, C), SIZES, neuron_type=sh["kind"], dropout=0.1, normalization="batchnorm").to(dev).train()
        loss_fn = Fn.CrossEntropyLoss()
        g = torch.Generator().manual_seed(2)
        y = torch.randint(0, SIZES[-1], (B,), generator=g).to(dev)
        x = (torch.rand(B, T, C, generator=torch.Generator().manual_seed(3)) < 0.05).float().to(dev)
        Tc = T // CHUNKS
        parts = [x[:, t0:t0 + Tc].contiguous() for t0 in range(0, T, Tc)]
        drawn = net.draw_states(B, dev)
        drawn.wait_ready()
        state0 = []
        for st in drawn:
            if isinstance(st, tuple):
                state0.append({k: v for k, v in zip(("u", "w", "s"), st) if v is not None})
            else:
                state0.append({"u": st})
        # a first state that wants its gradient (b, c), and a fixed linear form of the final state for the loss
        state_g = [{k: v.clone().requires_grad_(True) for k, v in st.items()} for st in state0]
        coef = [{k: torch.rand_like(v) for k, v in st.items()} for st in state0]

        def state_term(state):
            return sum((st[k] * c[k]).sum() for st, c in zip(state, coef) for k in st)

        torch.cuda.synchronize()

        def step(m):
            net.zero_grad(set_to_none=True)
            if m == "a":
                out, rates = net(x)
                loss_fn(out, y).backward()
            elif m == "b":
                for st in state_g:
                    for v in st.values():
                        v.grad = None
                out, rates, state = net(x, state=state_g, return_state=True)
                (loss_fn(out, y) + state_term(state)).backward()
            elif m == "c":
                for st in state_g:
                    for v in st.values():
                        v.grad = None
                state, total = state_g, 0
                for part in parts:
                    out, rates, state = net(part, state=state, return_state=True)
                    total = total + out
                (loss_fn(total, y) + state_term(state)).backward()
            else:
                state = state0
                for part in parts:
                    out, rates, state = net(part, state=state, return_state=True)
                    state = detach_state(state)
                    loss_fn(out, y).backward()

        for m in MODES:  # warm-up: allocator pools, kernel attributes
            for _ in range(3):
                step(m)
        Fn.check_status(dev)
        runs = {m: [] for m in MODES}
        for rep in range(args.reps):
            for m in MODES:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(m)
                torch.cuda.synchronize()
                runs[m].append(1e3 * (time.perf_counter() - t0) / args.steps)
        Fn.check_status(dev)
        med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
        for m in MODES:
            rec = {"shape": name, **sh, "mode": m, "chunks": 1 if m in "ab" else CHUNKS, "steps": args.steps,
                   "reps": args.reps, "ms_per_step": [round(v, 4) for v in runs[m]]}
            if m == "a":
                rec["spread_of_a"] = round((max(runs["a"]) - min(runs["a"])) / med(runs["a"]), 4)
            else:
                rec["ratio_to_a"] = round(med(runs[m]) / med(runs["a"]), 4)
            lines.append(rec)
            print(json.dumps(rec))
        del net
    with open(args.out, "w") as f:
        f.write("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
