"""
SHD / SSC loader with the reference's API (sparch/dataloaders/spiking_datasets.py):
`SpikingDataset(dataset_name, data_folder, split, nb_steps=100)` and
`load_shd_or_ssc(dataset_name, data_folder, split, batch_size, nb_steps=100, shuffle=True, workers=0)`,
whose batches keep the `(x, xlens, y)` collate contract (spiking_datasets.py:80-87).

What differs is WHERE the event lists become dense spike counts: the reference bins every sample on the
CPU (np.digitize + sparse -> dense, lines 66-78) and the trainer then uploads 280 KB per sample; here
`__getitem__` hands the raw `(times, units, label)` of a sample to the collate function, which uploads the
event lists (8 bytes per event) and bins the whole batch on the device with `sparch_bin_events` — the same
arithmetic (bit-exact against np.digitize + accumulate, tests/test_hip_parity.py::test_bin_events_*).
`dense_sample(index)` returns the reference's per-sample dense tensor for callers that want it.

h5py is imported when a dataset is opened (it is not installed in the offline build image: the class then
raises ImportError naming the package — there is no other source for the files' contents).

SPARCH_EVENTS=resident (or `load_shd_or_ssc(..., resident="resident")`) keeps the whole split on the device
instead (`functional.EventStore`): the events are uploaded once, and every batch is built there from the list
of its sample indices by one kernel (`sparch_events_gather_bin`) — no per-sample reads, no per-batch upload
but the indices of an epoch.  The index lists come from a torch DataLoader built with the arguments of the
per-sample loader, so the batches and the draws from torch's global generator are the same.  The events come
from the `h5_file` hook, else from the pack file `{data_folder}/{dataset}_{split}.events.npz`
(tools/pack_events.py; readable without h5py), else from the .h5 file.

`augment=SPEC` (resident loader only; `event_augment.py`): every epoch draws one table row per sample — channel
shift, time stretch and offset, event / window / band dropping — from a numpy generator seeded with
(augment_seed, rank, epoch number), uploads the table beside the index lists, and the batch kernel applies row b to
the events of batch row b while it bins them (`sparch_events_gather_bin_aug`).
"""
import logging
import os

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from ..functional import EventStore, bin_events
from ._index import _index_loader, _SampleIndices  # noqa: F401  (shared with the HD / SC loader)
from .event_augment import draw_event_augmentation, parse_event_augment

logger = logging.getLogger(__name__)


def _open_h5(filename):
    try:
        import h5py
    except ImportError as e:  # pragma: no cover - depends on the environment
        raise ImportError("sparch_amd.dataloaders: reading SHD/SSC needs the h5py package "
                          f"(file {filename})") from e
    return h5py.File(filename, "r")


class SpikingDataset(Dataset):
    """spiking_datasets.py:24-87.  `h5_file` (test hook): any mapping with ["spikes"]["times"],
    ["spikes"]["units"] and ["labels"] laid out like the dataset files."""

    def __init__(self, dataset_name, data_folder, split, nb_steps=100, h5_file=None, device="cuda"):
        self.device = device
        self.nb_steps = nb_steps
        self.nb_units = 700
        self.max_time = 1.4
        self.time_bins = np.linspace(0, self.max_time, num=self.nb_steps)
        filename = f"{data_folder}/{dataset_name}_{split}.h5"
        self.h5py_file = h5_file if h5_file is not None else _open_h5(filename)
        self.firing_times = self.h5py_file["spikes"]["times"]
        self.units_fired = self.h5py_file["spikes"]["units"]
        self.labels = np.array(self.h5py_file["labels"], dtype=np.int64)  # np.int in the reference (line 61)

    def __len__(self):
        return len(self.labels)

    def __getitem__(self, index):
        """Raw events of one sample: (times float32[n], units int32[n], label)."""
        return (np.asarray(self.firing_times[index], np.float32), np.asarray(self.units_fired[index], np.int32),
                int(self.labels[index]))

    def dense_sample(self, index):
        """The reference's `__getitem__` result (lines 66-78): (dense (nb_steps, nb_units) float32 on the
        CPU, label) — host-side, for inspection; the training path does not use it."""
        times = np.digitize(self.firing_times[index], self.time_bins)
        units = np.asarray(self.units_fired[index], np.int64)
        x = torch.zeros(self.nb_steps, self.nb_units)
        x.index_put_((torch.from_numpy(times.astype(np.int64)), torch.from_numpy(units)),
                     torch.ones(len(times)), accumulate=True)
        return x, int(self.labels[index])

    def generateBatch(self, batch):
        """(xs (B, nb_steps, nb_units) on the device, xlens (B,), ys (B,)) — spiking_datasets.py:80-87 with
        the binning done once per batch on the device."""
        times, units, ys = zip(*batch)
        xs, _ = bin_events(times, units, self.nb_steps, self.nb_units, self.max_time, device=self.device)
        xlens = torch.tensor([self.nb_steps] * len(ys))
        return xs, xlens, torch.LongTensor(ys)


class ResidentEventLoader:
    """Batches `(x, xlens, y)` of an `EventStore`: x and y on the device, xlens as the per-sample loader gives
    them.  Iterating draws the epoch's index lists from a DataLoader over the sample numbers (so `len`, the
    short last batch, `.sampler` / `set_epoch` and the global generator behave as with the per-sample loader),
    uploads them in one copy and launches one kernel per batch.  `values=True` asks for dense fp32 batches (a
    non-spiking network reads the values; a spiking one reads the bf16 plane the store serves when it can).
    `augment` (a spec of `event_augment.parse_event_augment`, text or parsed): every `__iter__` draws the whole
    epoch's table, one row per sample in the order the epoch serves them, from
    `np.random.default_rng([augment_seed, rank, epoch_index])`, epoch_index counting the iterations from 0; the
    table travels in one copy and each batch gets its slice.  Torch's global generator is not touched by it."""

    def __init__(self, store, batch_size, nb_steps=100, shuffle=True, rank=0, world=1, seed=0, values=False,
                 augment=None, augment_seed=0):
        self.store, self.batch_size, self.nb_steps, self.values = store, batch_size, nb_steps, values
        self.augment = parse_event_augment(augment) if augment is not None else None
        self.augment_seed, self.rank, self.epoch_index = int(augment_seed), int(rank), 0
        self.index_loader = _index_loader(_SampleIndices(len(store)), batch_size, shuffle, rank, world, seed)
        self.sampler = self.index_loader.sampler
        store.prepare(nb_steps)  # the one read-back the plane / fp32 decision needs: now, not in the first epoch

    def __len__(self):
        return len(self.index_loader)

    def index_lists(self):
        """The sample indices of every batch of one epoch (host tensors), in order."""
        return [b.to(torch.int64) for b in self.index_loader]

    def __iter__(self):
        lists = self.index_lists()
        if not lists:
            return
        flat = torch.cat(lists).to(self.store.device)
        table = seed = scale = None
        if self.augment is not None:
            rng = np.random.default_rng([self.augment_seed, self.rank, self.epoch_index])
            self.epoch_index += 1
            table, seed = draw_event_augmentation(flat.numel(), self.augment, rng, self.store.nb_units,
                                                  self.store.max_time)
            table, scale = self.store.upload_augmentation(table), self.augment["scale"]
        at = 0
        for b in lists:
            n = b.numel()
            if table is None:
                x, y = self.store.batch(flat[at:at + n], self.nb_steps, values=self.values)
            else:
                x, y = self.store.batch(flat[at:at + n], self.nb_steps, values=self.values,
                                        augment=(table[at:at + n], seed), augment_scale=scale)
            at += n
            yield x, torch.tensor([self.nb_steps] * n), y


def _event_pack_path(data_folder, dataset_name, split):
    return f"{data_folder}/{dataset_name}_{split}.events.npz"


def _resident_store(dataset_name, data_folder, split, h5_file, device):
    if h5_file is not None:
        return EventStore.from_mapping(h5_file, device=device)
    pack = _event_pack_path(data_folder, dataset_name, split)
    if os.path.exists(pack):
        return EventStore.from_pack(pack, device=device)
    with _open_h5(f"{data_folder}/{dataset_name}_{split}.h5") as f:
        return EventStore.from_mapping(f, device=device)


def load_shd_or_ssc(dataset_name, data_folder, split, batch_size, nb_steps=100, shuffle=True, workers=0,
                    h5_file=None, device="cuda", rank=0, world=1, seed=0, resident=None, values=False, augment=None,
                    augment_seed=0):
    """spiking_datasets.py:90-140.  rank / world (data-parallel runs; not in the reference, which is single
    device): every rank reads the same file and draws a disjoint 1/world share of each epoch's (shuffled)
    sample order through a DistributedSampler — call `loader.sampler.set_epoch(e)` per epoch; `batch_size`
    is the PER-RANK batch.  resident: None reads SPARCH_EVENTS; unset or empty = the per-sample loader,
    "resident" = a `ResidentEventLoader` (`values`, `augment`, `augment_seed`: see there); anything else is a
    ValueError, and so is `augment` with the per-sample loader."""
    if resident is None:
        resident = os.environ.get("SPARCH_EVENTS", "")
    if resident not in ("", "resident"):
        raise ValueError(f"SPARCH_EVENTS / resident: unknown value '{resident}' (unset or empty: per-sample "
                         "loader; 'resident': the split's events stay on the device)")
    if augment is not None:
        if resident != "resident":
            raise ValueError("augment: events are augmented inside the resident store's batch kernel; it needs "
                             "SPARCH_EVENTS=resident / resident='resident'")
        augment = parse_event_augment(augment)
    if dataset_name not in ["shd", "ssc"]:
        raise ValueError(f"Invalid dataset name {dataset_name}")
    if split not in ["train", "valid", "test"]:
        raise ValueError(f"Invalid split name {split}")
    if dataset_name == "shd" and split == "valid":
        logging.info("SHD does not have a validation split. Using test split.")
        split = "test"
    if workers != 0:
        raise ValueError("sparch_amd.dataloaders: the collate function bins on the GPU; use workers=0 "
                         "(the reference's default)")
    if resident == "resident":
        store = _resident_store(dataset_name, data_folder, split, h5_file, device)
        logging.info(f"Number of examples in {split} set: {len(store)}")
        loader = ResidentEventLoader(store, batch_size, nb_steps, shuffle, rank, world, seed, values=values,
                                     augment=augment, augment_seed=augment_seed)
        plane = store.serves_plane(nb_steps, augment["scale"] if augment is not None else None) and not values
        logging.info(f"Events of the {split} set are resident on {store.device}: {store.n_events} events, "
                     f"{store.nbytes / 2**20:.1f} MiB, times {'sorted' if store.sorted else 'unsorted'}, largest "
                     f"bin count {store.prepare(nb_steps)} ("
                     f"{'bf16 plane' if plane else 'dense fp32'} batches)")
        if augment is not None:
            logging.info(f"Events of the {split} set are augmented on the device: "
                         + ", ".join(f"{k}={v}" for k, v in augment.items() if v))
        if store.dropped(nb_steps):
            logging.warning(f"{store.dropped(nb_steps)} events of the {split} set are outside the {nb_steps} x "
                            f"{store.nb_units} grid and dropped (the reference's sparse constructor rejects them)")
        return loader
    dataset = SpikingDataset(dataset_name, data_folder, split, nb_steps, h5_file=h5_file, device=device)
    logging.info(f"Number of examples in {split} set: {len(dataset)}")
    return _index_loader(dataset, batch_size, shuffle, rank, world, seed, collate_fn=dataset.generateBatch)
