"""Resident SHD / SSC event store: kernel time per batch, host time per batch, and the training step on a pack.

The store is synthetic.  What it takes from the data sets: 700 channels, 1.4 s window, 100 time steps (the loader's
constants), float16 times and 16-bit units as the files store them, 20 classes, times ascending inside a sample
(the files list a sample's events in time order).  What it ASSUMES, because no SHD / SSC file was at hand to count:
the number of events per sample — log-normal around --events (default 8000, sigma 0.35) — and their spread: uniform
in time over the first 0.3-1.0 s of the window, channels from a per-sample band plus a uniform floor.  Kernel times
are also given at a quarter and at twice that density, so that the assumption's weight can be read off.

Reports (every pair alternates inside one process; medians and quartiles)
  * kernel time, HIP events around each call (and around 50 calls back to back, which leaves the launch gap out),
    B = --batch at 100 x 700 and 250 x 700: `sparch_events_gather_bin` writing the bf16 plane, against `sparch_bin_events` + `sparch_plane_bf16_exact` on the same batch with its
    events already uploaded (the per-sample loader's two passes; this change leaves their code as it was);
  * host time per batch over one epoch of the resident loader against the per-sample loader (`__getitem__` +
    `generateBatch`) and against `generateBatch` alone on pre-read samples, same mapping, shuffle off; "enqueue" is
    the time the host thread is busy, "through" includes the synchronise at the end of the epoch;
  * time per training step through `Experiment`, RadLIF 3 x 1024 at B = --batch, 100 time steps: SPARCH_EVENTS=
    resident on packs written from the store against --synthetic 1 (its bytes cross PCIe one batch ahead), epochs
    alternating, the first epoch of each is a warm-up.

    python tools/events_bench.py [--samples 4096] [--events 8000] [--out result.json]

--augment SPEC (dataloaders/event_augment.py, e.g. shift=40,scale=0.2,offset=0.1,drop=0.1,tmask=0.15,umask=70) reports
instead, and only, the kernel time of `sparch_events_gather_bin_aug` with rows drawn from SPEC alternating with
`sparch_events_gather_bin` on the same batches (B = --batch at 100 x 700 and 250 x 700, bf16 plane; the table is on
the device before the clock starts, as the loader uploads an epoch's table once).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NB_UNITS, MAX_TIME, N_CLASSES = 700, 1.4, 20


def synth_mapping(n_samples, events, seed=0):
    """A mapping laid out like an SHD file (rows are views into two flat arrays)."""
    g = np.random.default_rng(seed)
    lens = np.maximum(1, (events * g.lognormal(-0.5 * 0.35 ** 2, 0.35, n_samples)).astype(np.int64))
    off = np.zeros(n_samples + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    total = int(off[-1])
    sample = np.repeat(np.arange(n_samples), lens)
    dur = g.uniform(0.3, 1.0, n_samples)[sample]
    t = (g.random(total) * dur).astype(np.float16)
    band = g.integers(0, NB_UNITS - 200, n_samples)[sample]
    u = np.where(g.random(total) < 0.7, band + g.integers(0, 200, total), g.integers(0, NB_UNITS, total))
    order = np.argsort(sample + t.astype(np.float64) / 2, kind="stable")   # ascending times inside every sample
    t, u = t[order], u[order].astype(np.uint16)
    times = [t[off[i]:off[i + 1]] for i in range(n_samples)]
    units = [u[off[i]:off[i + 1]] for i in range(n_samples)]
    return {"spikes": {"times": times, "units": units}, "labels": g.integers(0, N_CLASSES, n_samples)}


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


def kernel_times(mapping, batch, nb_steps, reps, warmup):
    import torch

    from sparch_amd import functional as Fn
    from sparch_amd._capi import check, lib, ptr

    store = Fn.EventStore.from_mapping(mapping, device="cuda")
    g = torch.Generator().manual_seed(1)
    idx_h = torch.randperm(len(store), generator=g)[:batch]
    idx = idx_h.to("cuda")
    # the same batch as the per-sample loader uploads it: fp32 times, int32 units, offsets
    ts = [np.asarray(mapping["spikes"]["times"][i], np.float32) for i in idx_h.tolist()]
    us = [np.asarray(mapping["spikes"]["units"][i], np.int32) for i in idx_h.tolist()]
    offs = torch.zeros(batch + 1, dtype=torch.int64)
    offs[1:] = torch.cumsum(torch.tensor([len(t) for t in ts]), 0)
    t_d, u_d, o_d = (torch.from_numpy(np.concatenate(ts)).cuda(), torch.from_numpy(np.concatenate(us)).cuda(),
                     offs.cuda())
    n = int(offs[-1])
    dense = torch.empty(batch, nb_steps, NB_UNITS, device="cuda")
    dropped = torch.empty(4, dtype=torch.int32, device="cuda")
    keep = {}

    def resident():
        keep["new"] = store.gather(idx, nb_steps, plane=True)["plane"]

    def two_pass():
        check(lib.sparch_bin_events(n, ptr(t_d), ptr(u_d), ptr(o_d), batch, nb_steps, NB_UNITS, MAX_TIME, ptr(dense),
                                    ptr(dropped), torch.cuda.current_stream().cuda_stream), "sparch_bin_events")
        keep["old"] = Fn.plane_bf16_exact(dense.view(batch * nb_steps, NB_UNITS))[0]

    for _ in range(warmup):
        resident()
        two_pass()
    torch.cuda.synchronize()
    assert torch.equal(keep["new"].view(torch.int16), keep["old"].view(torch.int16)), "the two planes differ"
    new, old = [], []
    for _ in range(reps):
        new.append(_timed(resident))
        old.append(_timed(two_pass))
    def train_of(fn, k=50):   # k calls back to back inside one pair of events: the rate a training loop sees
        return _timed(lambda: [fn() for _ in range(k)]) / k

    new_b2b = [train_of(resident) for _ in range(5)]
    old_b2b = [train_of(two_pass) for _ in range(5)]
    plane_bytes = batch * nb_steps * ((NB_UNITS + 7) // 8 * 8) * 2
    return dict(events_in_batch=n, plane_bytes=plane_bytes, gather_bin_ms=_quartiles(new),
                bin_events_plus_plane_ms=_quartiles(old), gather_bin_back_to_back_ms=float(np.median(new_b2b)),
                bin_events_plus_plane_back_to_back_ms=float(np.median(old_b2b)),
                gather_bin_plane_write_GBps=plane_bytes / (np.median(new_b2b) * 1e-3) / 1e9)


def augment_kernel_times(mapping, batch, nb_steps, reps, warmup, spec):
    """Augmented and plain gather-and-bin on the same index list, alternating; both write the bf16 plane."""
    import torch

    from sparch_amd import functional as Fn
    from sparch_amd.dataloaders.event_augment import draw_event_augmentation

    store = Fn.EventStore.from_mapping(mapping, device="cuda")
    g = torch.Generator().manual_seed(1)
    idx = torch.randperm(len(store), generator=g)[:batch].to("cuda")
    table, seed = draw_event_augmentation(batch, spec, np.random.default_rng(1), NB_UNITS, MAX_TIME)
    table_d = store.upload_augmentation(table)
    lost = {}

    def augmented():
        store.gather(idx, nb_steps, plane=True, augment=(table_d, seed))

    def plain():
        store.gather(idx, nb_steps, plane=True)

    for _ in range(warmup):
        augmented()
        plain()
    for name, aug in (("augmented", (table_d, seed)), ("plain", None)):
        lost[name] = int(store.gather(idx, nb_steps, plane=True, dropped=True, augment=aug)["n_dropped"].item())
    new, old = [], []
    for _ in range(reps):
        new.append(_timed(augmented))
        old.append(_timed(plain))

    def train_of(fn, k=50):
        return _timed(lambda: [fn() for _ in range(k)]) / k

    new_b2b = [train_of(augmented) for _ in range(5)]
    old_b2b = [train_of(plain) for _ in range(5)]
    n = int((store.offsets[idx + 1] - store.offsets[idx]).sum().item())
    return dict(events_in_batch=n, events_not_placed=lost, gather_bin_aug_ms=_quartiles(new),
                gather_bin_ms=_quartiles(old), gather_bin_aug_back_to_back_ms=float(np.median(new_b2b)),
                gather_bin_back_to_back_ms=float(np.median(old_b2b)),
                aug_over_plain=float(np.median(new) / np.median(old)))


def host_times(mapping, batch, epochs):
    import torch

    from sparch_amd.dataloaders.spiking_datasets import SpikingDataset, load_shd_or_ssc

    res = {}
    loaders = {k: load_shd_or_ssc("shd", "/unused", "train", batch, shuffle=False, h5_file=mapping, device="cuda",
                                  resident=k) for k in ("", "resident")}
    rows = {k: dict(enqueue=[], through=[]) for k in ("per_sample", "resident", "generateBatch_only")}
    ds = SpikingDataset("shd", "/unused", "train", h5_file=mapping, device="cuda")
    pre = [[ds[i] for i in range(a, min(a + batch, len(ds)))] for a in range(0, len(ds), batch)]

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

    for e in range(epochs + 1):
        epoch("resident", lambda: iter(loaders["resident"]))
        epoch("per_sample", lambda: iter(loaders[""]))
        epoch("generateBatch_only", lambda: (ds.generateBatch(b) for b in pre))
    for k, v in rows.items():
        res[k] = dict(enqueue_ms_per_batch=_quartiles(v["enqueue"][1:]), through_ms_per_batch=_quartiles(v["through"][1:]))
    res["batches_per_epoch"] = len(pre)
    return res


def step_times(mapping, batch, epochs, tmp):
    import torch

    import pack_events
    import run_exp
    from sparch_amd.exp import Experiment

    data = os.path.join(tmp, "shd")
    os.makedirs(data)
    pack_events.pack_mapping(mapping, f"{data}/shd_train.events.npz")
    pack_events.pack_mapping(synth_mapping(batch, 2000, seed=9), f"{data}/shd_test.events.npz")
    n_batches = -(-len(mapping["labels"]) // batch)
    common = ["--model_type", "RadLIF", "--nb_layers", "3", "--nb_hiddens", "1024", "--dataset_name", "shd",
              "--batch_size", str(batch)]
    os.environ["SPARCH_EVENTS"] = "resident"
    try:
        on_pack = Experiment(run_exp.parse_args(common + ["--data_folder", data, "--new_exp_folder", f"{tmp}/e_pack"]))
    finally:
        os.environ.pop("SPARCH_EVENTS")
    synthetic = Experiment(run_exp.parse_args(common + ["--synthetic", "1", "--seq_len", "100", "--synthetic_batches",
                                                        str(n_batches), "--new_exp_folder", f"{tmp}/e_syn"]))
    rows = {"resident_pack": [], "synthetic": []}
    for e in range(1, epochs + 2):
        for name, exp in (("resident_pack", on_pack), ("synthetic", synthetic)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            exp.train_one_epoch(e)
            torch.cuda.synchronize()
            rows[name].append((time.perf_counter() - t0) * 1e3 / n_batches)
    res = {k: dict(ms_per_step=_quartiles(v[1:]), epochs=[round(x, 4) for x in v]) for k, v in rows.items()}
    res["steps_per_epoch"] = n_batches
    res["resident_over_synthetic"] = res["resident_pack"]["ms_per_step"]["median"] / res["synthetic"]["ms_per_step"]["median"]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--events", type=int, default=8000, help="assumed mean number of events per sample")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-epochs", type=int, default=3)
    ap.add_argument("--train-epochs", type=int, default=5)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--augment", default=None, metavar="SPEC",
                    help="time only the augmenting kernel against the plain one on the same batches")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch

    assert torch.cuda.is_available(), "events_bench needs a HIP device"
    res = dict(samples=a.samples, events_per_sample_assumed=a.events, batch=a.batch)
    mapping = synth_mapping(a.samples, a.events)
    if a.augment is not None:
        from sparch_amd.dataloaders.event_augment import parse_event_augment

        res["augment"] = {k: v for k, v in parse_event_augment(a.augment).items() if v}
        for nb_steps in (100, 250):
            r = augment_kernel_times(mapping, a.batch, nb_steps, a.reps, a.warmup, a.augment)
            res[f"augment_kernel_{a.events}ev_{nb_steps}x{NB_UNITS}"] = r
            print(f"kernel B={a.batch} {nb_steps}x{NB_UNITS}, {r['events_in_batch']} events: gather_bin_aug "
                  f"{r['gather_bin_aug_ms']['median']:.4f} ms [{r['gather_bin_aug_ms']['p25']:.4f}, "
                  f"{r['gather_bin_aug_ms']['p75']:.4f}] (back to back {r['gather_bin_aug_back_to_back_ms']:.4f} ms), "
                  f"gather_bin {r['gather_bin_ms']['median']:.4f} ms [{r['gather_bin_ms']['p25']:.4f}, "
                  f"{r['gather_bin_ms']['p75']:.4f}] (back to back {r['gather_bin_back_to_back_ms']:.4f} ms)",
                  flush=True)
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    for events in (a.events // 4, a.events, a.events * 2):
        m = mapping if events == a.events else synth_mapping(max(a.batch, 512), events, seed=events)
        for nb_steps in (100, 250):
            r = kernel_times(m, a.batch, nb_steps, a.reps, a.warmup)
            res[f"kernel_{events}ev_{nb_steps}x{NB_UNITS}"] = r
            print(f"kernel B={a.batch} {nb_steps}x{NB_UNITS}, {r['events_in_batch']} events: gather_bin "
                  f"{r['gather_bin_ms']['median']:.4f} ms (back to back {r['gather_bin_back_to_back_ms']:.4f} ms, "
                  f"{r['gather_bin_plane_write_GBps']:.0f} GB/s of plane), bin_events + plane_bf16_exact "
                  f"{r['bin_events_plus_plane_ms']['median']:.4f} ms (back to back "
                  f"{r['bin_events_plus_plane_back_to_back_ms']:.4f} ms)", flush=True)
    res["host"] = host_times(mapping, a.batch, a.host_epochs)
    for k in ("resident", "per_sample", "generateBatch_only"):
        h = res["host"][k]
        print(f"host {k}: enqueue {h['enqueue_ms_per_batch']['median']:.3f} ms per batch, through "
              f"{h['through_ms_per_batch']['median']:.3f} ms", flush=True)
    if not a.skip_train:
        with tempfile.TemporaryDirectory() as tmp:
            res["train"] = step_times(mapping, a.batch, a.train_epochs, tmp)
        t = res["train"]
        print(f"train step: resident on the pack {t['resident_pack']['ms_per_step']['median']:.3f} ms, --synthetic 1 "
              f"{t['synthetic']['ms_per_step']['median']:.3f} ms, ratio {t['resident_over_synthetic']:.3f}", flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
