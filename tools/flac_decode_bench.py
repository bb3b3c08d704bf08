"""FLAC decoding on the device: kernel time per batch and host time of the HD collate, FLAC against WAV.

Encodes N synthetic 48 kHz 16-bit mono clips with the test encoder (tests/flac_writer.py) at settings typical of
`flac -5` (4096-sample blocks, LPC order 8, 12-bit coefficients, partition order 4, Rice parameters per partition),
writes them as an HD tree of .flac files and the same tree as .wav, then reports
  * kernel time: sparch_flac_decode_padded on the already uploaded batch (its three kernels and memsets), HIP events
    around each launch, median and quartiles of --reps launches in one process after --warmup;
  * host time per batch: __getitem__ of every clip plus the collate function (no synchronisation; the first batch,
    which checks MD5 and synchronises, is a warm-up), median of --host-reps, for FLAC and for WAV;
  * the same at --long seconds per clip, to show how the host time scales with files and with samples.

    python tools/flac_decode_bench.py [--clips 256] [--seconds 1] [--long 4] [--out result.json]
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

RATE = 48000


def synth(n, seed):
    """A voiced-like clip: a few harmonics with a slow pitch glide and an envelope, plus low noise."""
    g = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    f0 = g.uniform(90, 220) * (1 + 0.1 * np.sin(2 * np.pi * 0.7 * t))
    ph = 2 * np.pi * np.cumsum(f0) / RATE
    x = sum(g.uniform(0.05, 0.3) / k * np.sin(k * ph + g.uniform(0, 6.3)) for k in range(1, 8))
    x = x * (0.3 + 0.7 * np.sin(np.pi * t / t[-1]) ** 2) + 0.003 * g.standard_normal(n)
    return np.clip(np.round(x * 32767), -32768, 32767).astype(np.int64)


def write_trees(root, n_clips, seconds):
    from tests import flac_writer as fw
    from tests.audio_trees import write_pcm_wav
    plan = lambda f, c, b: dict(kind="lpc", order=8, precision=12, porder=4)   # noqa: E731
    names, sizes = [], []
    for kind in ("flac", "wav"):
        os.makedirs(os.path.join(root, kind, "audio"), exist_ok=True)
    for k in range(n_clips):
        x = synth(int(seconds * RATE), k)
        stem = f"lang-english_speaker-{k % 10:02d}_trial-{k}_digit-{k % 10}"
        data = fw.write_flac(os.path.join(root, "flac", "audio", stem + ".flac"), x, 16, RATE, blocks=4096,
                             plan=plan)
        write_pcm_wav(os.path.join(root, "wav", "audio", stem + ".wav"), x.astype(np.int16), 2, RATE)
        names.append(stem)
        sizes.append(len(data))
    for kind in ("flac", "wav"):
        with open(os.path.join(root, kind, "train_filenames.txt"), "w") as f:
            f.write("".join(f"{s}.{kind}\n" for s in names))
    return sizes


def kernel_times(root, reps, warmup):
    import torch

    from sparch_amd import functional as Fn
    from sparch_amd._capi import check, lib
    from sparch_amd.dataloaders.audio import read_clip
    from sparch_amd.dataloaders.nonspiking_datasets import HeidelbergDigits
    ds = HeidelbergDigits(root, "train", False, 0.0001, 0.9, 0.1)
    clips = [read_clip(p)[0] for p in ds.file_list]
    ld = max(c.info.total_samples for c in clips)
    wave = torch.empty(len(clips), ld, dtype=torch.int16, device="cuda")
    host, table, n_slots, n_scratch = Fn.flac_pack([c.data for c in clips], [c.info for c in clips],
                                                  list(range(len(clips))), len(clips), ld, True)
    bytes_d, table_d = host.cuda(), torch.from_numpy(table).cuda()
    ws_bytes = lib.sparch_flac_workspace_bytes(n_slots, n_scratch)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    err = torch.empty(2, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        check(lib.sparch_flac_decode_padded(len(clips), table_d.data_ptr(), bytes_d.data_ptr(), host.numel(),
                                            n_slots, n_scratch, len(clips), ld, 1, wave.data_ptr(), err.data_ptr(),
                                            ws.data_ptr(), ws_bytes, stream), "sparch_flac_decode_padded")

    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    if int(err[0]) != 0:
        raise RuntimeError(f"decode errors: {err.tolist()}")
    for i, c in enumerate(clips[:8]):   # spot check against the WAV copy
        ref = np.frombuffer(open(ds.file_list[i].replace("/flac/", "/wav/")[:-5] + ".wav", "rb").read()[44:], "<i2")
        assert np.array_equal(wave[i, :c.info.total_samples].cpu().numpy(), ref), i
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    q = np.percentile(ms, [25, 50, 75])
    return dict(kernel_ms_p25=q[0], kernel_ms_median=q[1], kernel_ms_p75=q[2], frames=n_slots,
                bytes=int(host.numel()), samples=int(sum(c.info.total_samples for c in clips)))


def host_times(root, reps):
    import torch

    from sparch_amd.dataloaders.nonspiking_datasets import HeidelbergDigits
    ds = HeidelbergDigits(root, "train", False, 0.0001, 0.9, 0.1)
    ds._rate_warned = True
    out = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch = [ds[i] for i in range(len(ds))]
        t1 = time.perf_counter()
        xs, _, _ = ds.generateBatch(batch)
        t2 = time.perf_counter()
        torch.cuda.synchronize()
        ds.check_decode_errors()
        if r:  # the first batch is a warm-up (and checks MD5)
            out.append((t1 - t0, t2 - t1))
    get = statistics.median(a for a, _ in out) * 1e3
    col = statistics.median(b for _, b in out) * 1e3
    return dict(getitem_ms=get, collate_ms=col, host_ms=get + col)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--long", type=float, default=4.0, help="clip length of the scaling run (0: skip)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "flac_decode_bench needs a HIP device"
    res = dict(clips=a.clips, rate=RATE)
    with tempfile.TemporaryDirectory() as tmp:
        for tag, secs in (("short", a.seconds), ("long", a.long)):
            if secs <= 0:
                continue
            root = os.path.join(tmp, tag)
            t = time.perf_counter()
            sizes = write_trees(root, a.clips, secs)
            r = dict(seconds=secs, encode_s=time.perf_counter() - t,
                     flac_bytes_per_pcm_byte=sum(sizes) / (a.clips * secs * RATE * 2))
            r.update(kernel_times(os.path.join(root, "flac"), a.reps, a.warmup))
            r["flac"] = host_times(os.path.join(root, "flac"), a.host_reps)
            r["wav"] = host_times(os.path.join(root, "wav"), a.host_reps)
            res[tag] = r
            print(f"[{tag}] {a.clips} x {secs:g} s: kernel {r['kernel_ms_median']:.3f} ms "
                  f"(p25 {r['kernel_ms_p25']:.3f}, p75 {r['kernel_ms_p75']:.3f}; {r['frames']} frames); host per batch "
                  f"FLAC {r['flac']['host_ms']:.2f} ms (getitem {r['flac']['getitem_ms']:.2f} + collate "
                  f"{r['flac']['collate_ms']:.2f}), WAV {r['wav']['host_ms']:.2f} ms (getitem "
                  f"{r['wav']['getitem_ms']:.2f} + collate {r['wav']['collate_ms']:.2f}); FLAC/PCM bytes "
                  f"{r['flac_bytes_per_pcm_byte']:.2f}", flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
