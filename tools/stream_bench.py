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

--fused: the chunk of one step also through `StreamingSNN(fused=True)` (one launch per layer, csrc/streamstep.hip).  At
Tc = 1 the four modes eager / graph / fused / fused+graph are then timed stream by stream in turn (eager, graph, fused,
fused+graph, eager, ...), `--streams` streams each, and every row carries its own min and max over those streams;
a `fused_vs_unfused` line per B says whether both fused modes lie below the unfused rows' minimum by more than the
unfused rows' own min-max spread.  Defaults then: --batches 1 8 32 256, --out profiles/stream_bench_fused.jsonl.
Beside them, in the same turn-taking, the event-driven fused step `StreamingSNN(fused=True, sparse=True)`
(csrc/streamsparse.hip) as the modes sparse / sparse+graph, and the whole Tc = 1 block once per input density in
--densities (default 0.02 0.05 0.15; the hidden layers fire what the network at its initial parameters fires: every
row carries the measured firing rate per layer).  A `sparse_vs_fused` line per (B, density) claims a win only where the
sparse rows' MAX over the streams lies below the dense fused rows' MIN of the same call.

--ann: the non-spiking baselines of the same shape (MLP, RNN, LiGRU, GRU [1024, 1024, 35] on 700 channels, BatchNorm)
through `StreamingANN` (csrc/streamann.hip) at Tc = 1, eager and replayed, --batches 1 8 32 256.  Per (cell, B), taken
stream by stream in turn in one call: the two StreamingANN modes, the fused RadLIF stream eager and replayed, and the
whole-sequence eval forward `net(x)` at T = 250 of the same baseline — what a live stream had to re-run per step before
StreamingANN.  us per step as mean (min - max) over `--streams` streams after two warm-up streams; `lib_calls_per_step`
counted on the host as above.  No pass mark.  --out defaults to profiles/stream_bench_ann.jsonl.
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
    ap.add_argument("--fused", action="store_true", help="add the fused one-step path at Tc = 1 (see above)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", type=int, nargs="+", default=None)
    ap.add_argument("--chunks", type=int, nargs="+", default=[1, 10, 50, 250])
    ap.add_argument("--T", type=int, default=250)
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of whole forward / Tc = T stream")
    ap.add_argument("--streams", type=int, default=3, help="timed streams of T steps per (B, Tc, mode)")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 1024, 35])
    ap.add_argument("--channels", type=int, default=700)
    ap.add_argument("--densities", type=float, nargs="+", default=[0.02, 0.05, 0.15],
                    help="--fused: input densities of the Tc = 1 block (the other rows run at 0.05)")
    ap.add_argument("--ann", action="store_true", help="the non-spiking baselines through StreamingANN (see above)")
    args = ap.parse_args()
    if args.out is None:
        name = "stream_bench_ann.jsonl" if args.ann else "stream_bench_fused.jsonl" if args.fused else "stream_bench.jsonl"
        args.out = os.path.join(ROOT, "profiles", name)
    if args.batches is None:
        args.batches = [1, 8, 32, 256] if (args.fused or args.ann) else [1, 32, 256]

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

    def layer_rates(st):
        """Measured firing rate per hidden layer over all steps the stream has seen."""
        return [float(L.count[:L.H].sum()) / (st.batch_size * st.steps_seen * L.H) for L in st._layers if not L.readout]

    def fused_rows(B, chunks, density):
        """Tc = 1: the six modes, one stream each in turn, `--streams` times."""
        modes = {"eager": (False, False, False), "graph": (True, False, False), "fused": (False, True, False),
                 "fused+graph": (True, True, False), "sparse": (False, True, True), "sparse+graph": (True, True, True)}
        sts, calls, ms = {}, {}, {m: [] for m in modes}

        def stream(st):
            out = None
            for c in chunks:
                out = st.step(c)
            return out

        for mode, (graph, fused, sparse) in modes.items():
            st = sts[mode] = sparch_amd.StreamingSNN(net, B, graph=graph, fused=fused, sparse=sparse)
            st.reset()
            stream(st)                        # warm-up (graph: the eager pass, then the captures)
            stream(st)
            Fn.check_status(dev)
            calls[mode] = None if graph else count_calls(lambda: st.step(chunks[0]))
        for _ in range(args.streams):
            for mode in modes:
                ms[mode].append(timed(lambda: stream(sts[mode]), 1) / len(chunks))
        Fn.check_status(dev)
        for mode, (graph, fused, sparse) in modes.items():
            st, v = sts[mode], ms[mode]
            replayed = None if not graph else (bool(st._fg) and all(g["replays"] > 0 for g in st._fg.values())
                                               if fused else bool(st._g is not None))
            emit({"what": "stream", "B": B, "Tc": 1, "density": density, "mode": mode, "ms_per_chunk": sum(v) / len(v),
                  "ms_per_chunk_min": min(v), "ms_per_chunk_max": max(v), "ms_per_chunk_streams": v,
                  "us_per_step": 1e3 * sum(v) / len(v), "lib_calls_per_chunk": calls[mode], "graph_replayed": replayed,
                  "layer_firing_rates": layer_rates(st)})
        unf = ms["eager"] + ms["graph"]
        lo, spread = min(unf), max(max(ms["eager"]) - min(ms["eager"]), max(ms["graph"]) - min(ms["graph"]))
        emit({"what": "fused_vs_unfused", "B": B, "Tc": 1, "density": density, "unfused_min_ms": lo, "unfused_spread_ms": spread,
              "fused_max_ms": max(ms["fused"]), "fused_graph_max_ms": max(ms["fused+graph"]),
              "unfused_min_over_fused": lo / (sum(ms["fused"]) / len(ms["fused"])),
              "unfused_min_over_fused_graph": lo / (sum(ms["fused+graph"]) / len(ms["fused+graph"])),
              "fused_clears_margin": bool(max(ms["fused"]) < lo - spread),
              "fused_graph_clears_margin": bool(max(ms["fused+graph"]) < lo - spread)})
        emit({"what": "sparse_vs_fused", "B": B, "Tc": 1, "density": density,
              "fused_min_ms": min(ms["fused"]), "sparse_max_ms": max(ms["sparse"]),
              "fused_graph_min_ms": min(ms["fused+graph"]), "sparse_graph_max_ms": max(ms["sparse+graph"]),
              "fused_over_sparse": (sum(ms["fused"]) / len(ms["fused"])) / (sum(ms["sparse"]) / len(ms["sparse"])),
              "fused_graph_over_sparse_graph": (sum(ms["fused+graph"]) / len(ms["fused+graph"])) /
                                               (sum(ms["sparse+graph"]) / len(ms["sparse+graph"])),
              "sparse_wins": bool(max(ms["sparse"]) < min(ms["fused"])),
              "sparse_graph_wins": bool(max(ms["sparse+graph"]) < min(ms["fused+graph"])),
              "sparse_loses": bool(min(ms["sparse"]) > max(ms["fused"])),
              "sparse_graph_loses": bool(min(ms["sparse+graph"]) > max(ms["fused+graph"]))})

    def ann_rows(kind, B, x):
        """Tc = 1 on the `kind` baseline of the same shape: StreamingANN eager and replayed, the fused RadLIF stream
        eager and replayed, and the whole-sequence eval forward net(x) of the baseline (what there was before
        StreamingANN), one stream / forward each in turn, `--streams` times after two warm-up turns."""
        from sparch_amd.anns import ANN
        torch.manual_seed(1234)
        ann = ANN((B, None, C), args.sizes, ann_type=kind, normalization="batchnorm").to(dev).eval()
        chunks = [x[:, t0:t0 + 1] for t0 in range(T)]        # read where they lie
        sts = {"eager": sparch_amd.StreamingANN(ann, B), "graph": sparch_amd.StreamingANN(ann, B, graph=True),
               "radlif_fused": sparch_amd.StreamingSNN(net, B, fused=True),
               "radlif_fused+graph": sparch_amd.StreamingSNN(net, B, graph=True, fused=True)}

        def stream(st):
            out = None
            for c in chunks:
                out = st.step(c)
            return out

        def whole():
            with torch.no_grad():
                return ann(x)

        for st in sts.values():
            st.reset()
            stream(st)
            stream(st)
        whole(), whole()
        Fn.check_status(dev)
        calls = {m: count_calls(lambda st=st: st.step(chunks[0])) for m, st in sts.items() if not st.graph}
        us, whole_ms = {m: [] for m in sts}, []
        for _ in range(args.streams):
            for m, st in sts.items():
                us[m].append(1e3 * timed(lambda st=st: stream(st), 1) / T)
            whole_ms.append(timed(whole, 1))
        Fn.check_status(dev)
        for m, st in sts.items():
            v = us[m]
            graphs = getattr(st, "_fg", None) if m.startswith("radlif") else st._g
            emit({"what": "ann_stream" if not m.startswith("radlif") else "radlif_stream", "cell": kind, "B": B, "Tc": 1,
                  "mode": m, "us_per_step": sum(v) / len(v), "us_per_step_min": min(v), "us_per_step_max": max(v),
                  "us_per_step_streams": v, "lib_calls_per_step": calls.get(m),
                  "graph_replayed": (bool(graphs) and all(g["replays"] > 0 for g in graphs.values())) if st.graph else None})
        emit({"what": "ann_whole_forward", "cell": kind, "B": B, "T": T, "ms_per_forward": sum(whole_ms) / len(whole_ms),
              "ms_per_forward_min": min(whole_ms), "ms_per_forward_max": max(whole_ms), "ms_per_forward_calls": whole_ms,
              "us_per_step_equivalent": 1e3 * sum(whole_ms) / len(whole_ms) / T,
              "whole_forward_over_eager_step": sum(whole_ms) / len(whole_ms) * 1e3 / (sum(us["eager"]) / len(us["eager"]))})

    if args.ann:
        for kind in ("MLP", "RNN", "LiGRU", "GRU"):
            for B in args.batches:
                g = torch.Generator().manual_seed(4321 + B)
                ann_rows(kind, B, (torch.rand(B, T, C, generator=g) < 0.05).float().to(dev))
        args.batches = []

    for B in args.batches:
        g = torch.Generator().manual_seed(4321 + B)
        x = (torch.rand(B, T, C, generator=g) < 0.05).float().to(dev)

        def whole():
            with torch.no_grad():
                return net(x)

        for Tc in args.chunks:
            chunks = [x[:, t0:t0 + Tc].contiguous() for t0 in range(0, T, Tc)]
            if args.fused and Tc == 1:
                for density in args.densities:
                    gd = torch.Generator().manual_seed(4321 + B + int(round(1000 * density)))
                    xd = (torch.rand(B, T, C, generator=gd) < density).float().to(dev)
                    fused_rows(B, [xd[:, t0:t0 + 1].contiguous() for t0 in range(T)], density)
                continue
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
