#!/usr/bin/env python
"""Streaming inference against the whole-sequence eval forward, on the headline network.

RadLIF [1024, 1024, 35] on 700 input channels (0/1 spikes, 5 % rate), B in {1, 32, 256}, chunk lengths Tc in
{1, 10, 50, 250}: a stream of T = 250 steps is pushed through `StreamingSNN.step` in chunks of Tc, eager and with
graph=True (the replayed captured step), and timed with device events around whole streams after a warmed-up stream
of the same shape (graph: warmed up until the step has been captured, so no timed call holds the capture).  Reported
per (B, Tc, mode): ms per chunk, us per time step, and for one eager chunk step `lib_calls_per_chunk`: the C-ABI calls
counted on the host.  That is a lower bound of the launches, not their number: a call may launch more than one kernel
(the recurrent cell: a memset and the kernel; a split-K product: the product and its reduction), and torch's own
kernels (the state copy of the returned output, a pad of a width that is not a multiple of 4) are not in it.

In the same process, alternating with the Tc = 250 stream at each B: the existing eval forward `net(x)` over the
whole T = 250 sequence (fresh state draws, V pack, BatchNorm fold and W split per call, save tensors written by the
recurrent kernels), repeated `--rounds` times — its own min / max over the rounds is the spread a difference has to
exceed to mean anything.

One JSON object per line goes to --out (default profiles/stream_bench.jsonl) and to stdout.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench.jsonl"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--chunks", type=int, nargs="+", default=[1, 10, 50, 250])
    ap.add_argument("--T", type=int, default=250)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of whole forward / Tc = T stream")
    ap.add_argument("--streams", type=int, default=3, help="timed streams of T steps per (B, Tc, mode)")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 1024, 35])
    ap.add_argument("--channels", type=int, default=700)
    args = ap.parse_args()

    import torch

    import sparch_amd
    from sparch_amd import _capi
    from sparch_amd import functional as Fn

    if not torch.cuda.is_available():
        raise SystemExit("stream_bench: needs a HIP device (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    T, C = args.T, args.channels
    torch.manual_seed(1234)
    net = sparch_amd.SNN((max(args.batches), None, C), args.sizes, neuron_type="RadLIF", dropout=0.1,
                         normalization="batchnorm").to(dev).eval()
    lines = [{"what": "note", "lib_calls_per_chunk": "C-ABI calls of one eager chunk step, counted on the host: a lower "
              "bound of the kernel launches (a call may launch several kernels; torch's own kernels are not counted)"}]

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)

    def timed(fn, n):
        """ms per call of fn over n calls (device events; the work ends in a synchronise)."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    def count_calls(fn):
        """Library calls made by fn(): every bound entry point is wrapped for the duration."""
        names = [n for n in _capi.PROTOTYPES if not n.endswith("_bytes") and n not in ("sparch_device_cus",)]
        saved, n_calls = {}, [0]
        for name in names:
            f = getattr(_capi.lib, name)
            saved[name] = f

            def wrapped(*a, _f=f):
                n_calls[0] += 1
                return _f(*a)
            setattr(_capi.lib, name, wrapped)
        try:
            fn()
        finally:
            for name, f in saved.items():
                setattr(_capi.lib, name, f)
        return n_calls[0]

    for B in args.batches:
        g = torch.Generator().manual_seed(4321 + B)
        x = (torch.rand(B, T, C, generator=g) < 0.05).float().to(dev)

        def whole():
            with torch.no_grad():
                return net(x)

        for Tc in args.chunks:
            chunks = [x[:, t0:t0 + Tc].contiguous() for t0 in range(0, T, Tc)]
            for mode in ("eager", "graph"):
                st = sparch_amd.StreamingSNN(net, B, graph=(mode == "graph"))

                def stream(st=st, chunks=chunks):
                    out = None
                    for c in chunks:
                        out = st.step(c)
                    return out

                st.reset()
                stream()                      # warm-up (graph: eager passes, then the capture)
                stream()
                for _ in range(3):
                    if mode == "graph" and st._g is None:
                        stream()
                Fn.check_status(dev)
                calls = count_calls(lambda: st.step(chunks[0])) if mode == "eager" else None
                ms = timed(stream, args.streams)
                Fn.check_status(dev)
                emit({"what": "stream", "B": B, "Tc": Tc, "mode": mode, "ms_per_chunk": ms / len(chunks),
                      "us_per_step": 1e3 * ms / T, "ms_per_stream": ms, "lib_calls_per_chunk": calls,
                      "graph_replayed": bool(st._g is not None) if mode == "graph" else None})
        # whole-sequence eval forward against the Tc = T stream, alternating
        st = sparch_amd.StreamingSNN(net, B)
        st.reset()
        whole(), st.step(x), whole(), st.step(x)
        Fn.check_status(dev)
        w_ms, s_ms = [], []
        for _ in range(args.rounds):
            w_ms.append(timed(whole, 5))
            s_ms.append(timed(lambda: st.step(x), 5))
        Fn.check_status(dev)
        emit({"what": "whole_vs_stream", "B": B, "T": T, "whole_forward_ms": w_ms, "stream_TcT_ms": s_ms,
              "whole_min": min(w_ms), "whole_max": max(w_ms), "whole_spread": max(w_ms) - min(w_ms),
              "stream_min": min(s_ms), "stream_max": max(s_ms),
              "stream_no_slower": bool(min(s_ms) <= min(w_ms) + (max(w_ms) - min(w_ms))),
              "whole_lib_calls": count_calls(whole), "stream_lib_calls": count_calls(lambda: st.step(x))})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
