"""Waveform augmentation on the device: kernel time per batch, host time of the draws, and the SC collate with and
without augmentation.

Reports
  * kernel time: sparch_augment_padded on an uploaded (clips, samples) fp32 batch of synthetic speech-like clips,
    HIP events around each launch, median and quartiles of --reps launches after --warmup, at 16000 and 48000 samples
    per clip, (a) every stage on every clip (R = D = S = 99), (b) tables drawn with the reference's probabilities
    (p_noise 0.1) and (c) polarity, noise and gain on every clip, no reverb;
  * host time of dataloaders.augment.draw_augmentation per batch (median of --host-reps);
  * host time of the SC collate function on a tree of one-second 16-bit WAV clips (__getitem__ excluded, no
    synchronisation inside; the first batch is a warm-up), with SPARCH_AUGMENT=restated and without.

    python tools/augment_bench.py [--clips 256] [--out result.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth(n_clips, n, seed=0):
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    f0 = g.uniform(90, 220, (n_clips, 1))
    x = sum(g.uniform(0.05, 0.3, (n_clips, 1)) / k * np.sin(2 * np.pi * k * f0 * t + g.uniform(0, 6.3, (n_clips, 1)))
            for k in range(1, 8))
    return (x + 0.003 * g.standard_normal((n_clips, n))).astype(np.float32)


def kernel_times(n_clips, n, table, reps, warmup):
    import torch

    from sparch_amd._capi import check, lib
    wave = torch.from_numpy(synth(n_clips, n)).cuda()
    lens = torch.full((n_clips,), n, dtype=torch.int32, device="cuda")
    prm = torch.from_numpy(table).cuda()
    out = torch.empty_like(wave)
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        check(lib.sparch_augment_padded(n_clips, n, lens.data_ptr(), 0, wave.data_ptr(), prm.data_ptr(), 0.0001, 0.9,
                                        1234, 16000, out.data_ptr(), stream), "sparch_augment_padded")

    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    q = np.percentile(ms, [25, 50, 75])
    return dict(kernel_ms_p25=q[0], kernel_ms_median=q[1], kernel_ms_p75=q[2])


def draw_times(n_clips, reps):
    from sparch_amd.dataloaders.augment import draw_augmentation
    ts = []
    for _ in range(reps + 1):
        t = time.perf_counter()
        draw_augmentation(n_clips, 0.0001, 0.9, 0.1)
        ts.append(time.perf_counter() - t)
    return statistics.median(ts[1:]) * 1e3


def collate_times(root, n_clips, reps):
    import torch

    from sparch_amd.dataloaders.nonspiking_datasets import SpeechCommands
    res = {}
    for mode in ("", "restated"):
        os.environ["SPARCH_AUGMENT"] = mode
        ds = SpeechCommands(root, "training", mode != "", 0.0001, 0.9, 0.1)
        batch = [ds[i] for i in range(min(n_clips, len(ds)))]
        ts = []
        for r in range(reps + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            ds.generateBatch(batch)
            ts.append(time.perf_counter() - t)
        torch.cuda.synchronize()
        res["augmented_ms" if mode else "plain_ms"] = statistics.median(ts[1:]) * 1e3
    os.environ.pop("SPARCH_AUGMENT")
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import random

    import torch

    from sparch_amd.dataloaders.augment import draw_augmentation
    from tests.audio_trees import make_sc_tree
    assert torch.cuda.is_available(), "augment_bench needs a HIP device"
    random.seed(0)
    torch.manual_seed(0)
    np.random.seed(0)
    every = np.zeros((a.clips, 9), np.float32)
    every[:, :4] = 1
    every[:, 4], every[:, 5], every[:, 6:] = 0.5, 0.3, 99
    drawn = draw_augmentation(a.clips, 0.0001, 0.9, 0.1)[0]
    dry = every.copy()
    dry[:, 3] = 0
    res = dict(clips=a.clips)
    for n in (16000, 48000):
        for tag, table in (("all_stages", every), ("reference_p", drawn), ("no_reverb", dry)):
            r = kernel_times(a.clips, n, table, a.reps, a.warmup)
            res[f"kernel_{n}_{tag}"] = r
            print(f"kernel {a.clips} x {n} {tag}: {r['kernel_ms_median']:.3f} ms (p25 {r['kernel_ms_p25']:.3f}, "
                  f"p75 {r['kernel_ms_p75']:.3f})", flush=True)
    res["draw_ms"] = draw_times(a.clips, a.host_reps)
    print(f"draw_augmentation per {a.clips}-clip batch: {res['draw_ms']:.3f} ms", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        per_word = -(-a.clips // 3)
        make_sc_tree(tmp, n_train=per_word, n_valid=1, n_test=1)
        res["collate"] = collate_times(tmp, a.clips, a.host_reps)
    print(f"SC collate per batch: {res['collate']['plain_ms']:.2f} ms plain, "
          f"{res['collate']['augmented_ms']:.2f} ms augmented", flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
