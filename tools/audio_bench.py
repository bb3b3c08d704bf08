"""Resident HD / SC audio store: kernel time per batch, host time per batch, and the training step on a tree.

The clips are synthetic: a Speech Commands tree of --clips one-second 16-bit mono WAV files (a tone per word plus
noise) written to a temporary folder, so that the file loader pays its real per-file reads (page cache warm after the
first epoch).  Nothing here depends on what the clips sound like.

Reports (every pair alternates inside one process; medians and quartiles)
  * kernel time, HIP events around each call (and around 50 calls back to back, which leaves the launch gap out),
    B = --batch: `sparch_audio_gather_fbank` from the store against `sparch_fbank_padded_fwd` on the same clips as an
    already-uploaded int16 batch buffer — the same per-frame device code; outputs are compared bit for bit first;
    and the gather kernel once more on a store holding the same clips at odd, mutually different start offsets;
  * host time per batch over one epoch, shuffle off: the resident loader against the file loader (`__getitem__` +
    `generateBatch`), and the file loader's two halves on their own — reading the clips of a batch (`__getitem__`),
    and `generateBatch` on pre-read clips; "enqueue" is the time the host thread is busy, "through" includes the
    synchronise at the end of the epoch;
  * time per training step through `Experiment`, RadLIF 3 x 1024 at B = --batch: SPARCH_AUDIO=resident against the
    file loader on the same tree and against --synthetic 1, epochs alternating, the first epoch of each is a warm-up.

    python tools/audio_bench.py [--clips 4096] [--out result.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATE = 16000
WORDS = ("down", "go", "left", "no", "off", "on", "right", "stop", "up", "yes")


def write_tree(root, n_clips, n_eval=64, seed=0):
    """Speech Commands layout: _background_noise_, one folder per word, validation_list.txt, testing_list.txt."""
    g = np.random.default_rng(seed)
    t = np.arange(RATE) / RATE

    def clip(word):
        x = 0.3 * np.sin(2 * np.pi * (200.0 + 170.0 * word) * t + g.uniform(0, 6.28)) + 0.05 * g.uniform(-1, 1, RATE)
        return np.round(x * 32767).astype("<i2")

    def put(path, pcm):
        with wave.open(path, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(RATE)
            w.writeframes(pcm.tobytes())

    os.makedirs(os.path.join(root, "_background_noise_"))
    put(os.path.join(root, "_background_noise_", "noise.wav"), clip(0))
    lists = {"validation": [], "testing": []}
    for w, word in enumerate(WORDS):
        os.makedirs(os.path.join(root, word))
    for i in range(n_clips + 2 * n_eval):
        w = i % len(WORDS)
        name = f"{WORDS[w]}/{i:06d}_nohash_0.wav"
        put(os.path.join(root, name), clip(w))
        if i >= n_clips:
            lists["validation" if (i - n_clips) % 2 == 0 else "testing"].append(name)
    for k, names in lists.items():
        with open(os.path.join(root, f"{k}_list.txt"), "w") as f:
            f.write("".join(n + "\n" for n in names))


def _quartiles(ms):
    q = np.percentile(ms, [25, 50, 75])
    return dict(p25=float(q[0]), median=float(q[1]), p75=float(q[2]))


def _timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_times(store, batch, reps, warmup):
    import torch

    from sparch_amd._capi import check, lib, ptr

    g = torch.Generator().manual_seed(1)
    idx_h = torch.randperm(len(store), generator=g)[:batch]
    idx = idx_h.to("cuda")
    lens_h = store.lengths_host[idx_h]
    ld = int(lens_h.max())
    n_frames = lib.sparch_fbank_frames(ld)
    # the same clips as the file loader uploads them: one (batch, ld) buffer and their lengths
    at = store.starts[idx][:, None] + torch.arange(ld, device="cuda")[None]
    wave_d = store.samples[at.clamp(max=store.n_samples - 1)].contiguous()
    lens_d = lens_h.to(torch.int32).to("cuda")
    out_old = torch.empty(batch, n_frames, 40, device="cuda")
    keep = {}
    # the same clips once more in a store whose clip i starts 2 i + 1 samples later (odd starts, no two clips aligned
    # alike): what leaving the clips unaligned costs the gather kernel
    from sparch_amd.functional import AudioStore

    a = {k: getattr(store, k).cpu().numpy() for k in ("samples", "starts", "lengths", "labels")}
    shift = 2 * np.arange(len(store), dtype=np.int64) + 1
    shift = np.cumsum(shift)
    moved = np.zeros(len(a["samples"]) + int(shift[-1]), a["samples"].dtype)
    for s0, n0, d in zip(a["starts"], a["lengths"], shift):
        moved[s0 + d:s0 + d + n0] = a["samples"][s0:s0 + n0]
    odd = AudioStore(dict(a, samples=moved, starts=a["starts"] + shift), device="cuda")
    assert int((odd.starts % 2).sum()) > 0

    def resident_odd():
        keep["odd"] = odd.gather_fbank(idx, n_frames)[0]

    def resident():
        keep["new"] = store.gather_fbank(idx, n_frames)[0]

    def padded():
        check(lib.sparch_fbank_padded_fwd(batch, ld, ptr(lens_d), n_frames, 40, store.dtype, ptr(wave_d), ptr(out_old),
                                          torch.cuda.current_stream().cuda_stream), "sparch_fbank_padded_fwd")

    for _ in range(warmup):
        resident()
        padded()
        resident_odd()
    torch.cuda.synchronize()
    assert torch.equal(keep["new"].view(torch.int32), out_old.view(torch.int32)), "the two feature tensors differ"
    assert torch.equal(keep["odd"].view(torch.int32), out_old.view(torch.int32)), "odd starts change the features"
    new, old, unaligned = [], [], []
    for _ in range(reps):
        new.append(_timed(resident))
        old.append(_timed(padded))
        unaligned.append(_timed(resident_odd))

    def train_of(fn, k=50):   # k calls back to back inside one pair of events: the rate a training loop sees
        return _timed(lambda: [fn() for _ in range(k)]) / k

    new_b2b, old_b2b, odd_b2b = [], [], []
    for _ in range(5):
        new_b2b.append(train_of(resident))
        old_b2b.append(train_of(padded))
        odd_b2b.append(train_of(resident_odd))
    return dict(batch=batch, samples_per_clip=ld, frames=n_frames, reps=reps, gather_fbank_ms=_quartiles(new),
                fbank_padded_ms=_quartiles(old), gather_fbank_odd_starts_ms=_quartiles(unaligned),
                gather_fbank_odd_starts_back_to_back_ms=float(np.median(odd_b2b)),
                gather_fbank_back_to_back_ms=float(np.median(new_b2b)),
                fbank_padded_back_to_back_ms=float(np.median(old_b2b)))


def host_times(root, batch, epochs):
    import torch

    from sparch_amd.dataloaders.nonspiking_datasets import load_hd_or_sc

    loaders = {k: load_hd_or_sc("sc", root, "train", batch, shuffle=False, device="cuda", resident=k)
               for k in ("", "resident")}
    ds = loaders[""].dataset
    chunks = [range(a, min(a + batch, len(ds))) for a in range(0, len(ds), batch)]
    pre = [[ds[i] for i in c] for c in chunks]
    rows = {k: dict(enqueue=[], through=[]) for k in ("file_loader", "resident", "read_clips_only",
                                                      "generateBatch_only")}

    def epoch(name, it):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 0
        for _ in it():
            n += 1
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        rows[name]["enqueue"].append((t1 - t0) * 1e3 / n)
        rows[name]["through"].append((t2 - t0) * 1e3 / n)

    for _ in range(epochs + 1):
        epoch("resident", lambda: iter(loaders["resident"]))
        epoch("file_loader", lambda: iter(loaders[""]))
        epoch("read_clips_only", lambda: ([ds[i] for i in c] for c in chunks))
        epoch("generateBatch_only", lambda: (ds.generateBatch(b) for b in pre))
    res = {k: dict(enqueue_ms_per_batch=_quartiles(v["enqueue"][1:]), through_ms_per_batch=_quartiles(v["through"][1:]))
           for k, v in rows.items()}
    res["batches_per_epoch"] = len(chunks)
    res["epochs"] = epochs
    return res, loaders["resident"].store


def step_times(root, batch, n_clips, epochs, tmp):
    import torch

    import run_exp
    from sparch_amd.exp import Experiment

    n_batches = -(-n_clips // batch)
    common = ["--model_type", "RadLIF", "--nb_layers", "3", "--nb_hiddens", "1024", "--dataset_name", "sc",
              "--batch_size", str(batch)]
    os.environ["SPARCH_AUDIO"] = "resident"
    try:
        resident = Experiment(run_exp.parse_args(common + ["--data_folder", root, "--new_exp_folder", f"{tmp}/e_res"]))
    finally:
        os.environ.pop("SPARCH_AUDIO")
    files = Experiment(run_exp.parse_args(common + ["--data_folder", root, "--new_exp_folder", f"{tmp}/e_files"]))
    synthetic = Experiment(run_exp.parse_args(common + ["--synthetic", "1", "--synthetic_batches", str(n_batches),
                                                        "--new_exp_folder", f"{tmp}/e_syn"]))
    rows = {"resident": [], "file_loader": [], "synthetic": []}
    for e in range(1, epochs + 2):
        for name, exp in (("resident", resident), ("file_loader", files), ("synthetic", synthetic)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            exp.train_one_epoch(e)
            torch.cuda.synchronize()
            rows[name].append((time.perf_counter() - t0) * 1e3 / n_batches)
    res = {k: dict(ms_per_step=_quartiles(v[1:]), epochs=[round(x, 4) for x in v]) for k, v in rows.items()}
    res["steps_per_epoch"] = n_batches
    med = {k: res[k]["ms_per_step"]["median"] for k in rows}
    res["resident_over_synthetic"] = med["resident"] / med["synthetic"]
    res["file_loader_over_resident"] = med["file_loader"] / med["resident"]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-epochs", type=int, default=3)
    ap.add_argument("--train-epochs", type=int, default=5)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    assert torch.cuda.is_available(), "audio_bench needs a HIP device"
    res = dict(clips=a.clips, batch=a.batch, samples_per_clip=RATE)
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "sc")
        write_tree(root, a.clips)
        res["host"], store = host_times(root, a.batch, a.host_epochs)
        for k in ("resident", "file_loader", "read_clips_only", "generateBatch_only"):
            h = res["host"][k]
            print(f"host {k}: enqueue {h['enqueue_ms_per_batch']['median']:.3f} ms per batch, through "
                  f"{h['through_ms_per_batch']['median']:.3f} ms", flush=True)
        res["store_MiB"] = store.nbytes / 2**20
        r = res["kernel"] = kernel_times(store, a.batch, a.reps, a.warmup)
        print(f"kernel B={a.batch} x {r['samples_per_clip']} samples: gather_fbank {r['gather_fbank_ms']['median']:.4f} "
              f"ms (back to back {r['gather_fbank_back_to_back_ms']:.4f} ms), fbank_padded "
              f"{r['fbank_padded_ms']['median']:.4f} ms (back to back {r['fbank_padded_back_to_back_ms']:.4f} ms), "
              f"gather_fbank with odd clip starts {r['gather_fbank_odd_starts_ms']['median']:.4f} ms (back to back "
              f"{r['gather_fbank_odd_starts_back_to_back_ms']:.4f} ms)",
              flush=True)
        del store
        if not a.skip_train:
            t = res["train"] = step_times(root, a.batch, a.clips, a.train_epochs, tmp)
            print(f"train step: resident {t['resident']['ms_per_step']['median']:.3f} ms, file loader "
                  f"{t['file_loader']['ms_per_step']['median']:.3f} ms, --synthetic 1 "
                  f"{t['synthetic']['ms_per_step']['median']:.3f} ms; resident / synthetic "
                  f"{t['resident_over_synthetic']:.3f}, file loader / resident "
                  f"{t['file_loader_over_resident']:.3f}", flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
