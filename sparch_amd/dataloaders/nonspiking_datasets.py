"""
HD / SC loader with the reference's API (sparch/dataloaders/nonspiking_datasets.py):
`HeidelbergDigits(data_folder, split, use_augm, min_snr, max_snr, p_noise)`,
`SpeechCommands(data_folder, split, use_augm, min_snr, max_snr, p_noise)` and
`load_hd_or_sc(dataset_name, data_folder, split, batch_size, shuffle=True, use_augm=False, min_snr=0.0001,
max_snr=0.9, p_noise=0.1, workers=0)`, whose batches keep the `(xs, xlens, ys)` collate contract
(nonspiking_datasets.py:104-111, 202-209): xs (B, T_max, 40) log-mel features, padded with zeros after each
clip's own frames, xlens the frame counts, ys a LongTensor.

What differs is WHERE the features are made: the reference runs torchaudio's kaldi.fbank per clip on the CPU in
`__getitem__` and pads in the collate function; here `__getitem__` returns the decoded host samples of a WAV clip,
or the undecoded bytes and STREAMINFO of a FLAC clip (`audio.read_clip`), and the collate function packs the WAV
samples into one pinned buffer, uploads it (int16 when every clip is 16-bit mono), decodes the FLAC clips into
their rows of the same device buffer (`functional.flac_decode_padded`, one pinned upload of their bytes) and makes
the padded features with one kernel (`functional.fbank_padded`).

FLAC decode errors are found without a per-batch synchronisation: the error record is copied to pinned memory
behind an event, read when the next batch is collated if the event has completed, and at the end of the epoch at
the latest (FlacError naming the file).  On a dataset's first batch the decoded samples of every mono FLAC clip
with a non-zero STREAMINFO MD5 are copied back and hashed (one synchronising copy, once): a decoder that misreads
the format fails there instead of training on wrong audio.

File lists, their order and the labels are the reference's, with two of its bugs left out:
  * SC labels are the sorted subdirectories of `data_folder` minus the first (`_background_noise_` in the v0.02
    layout); the reference lists them with `os.walk("./" + data_folder)`, which breaks absolute paths;
  * the SC training split drops the files named in validation_list.txt and testing_list.txt; the reference
    compares path strings, which silently drops nothing when `data_folder` starts with "./".  Here paths are
    compared relative to `data_folder`.
Augmentation (`use_augm=True`) is an explicit opt-in.  The reference's transforms (torchaudio_augmentations, whose
Reverb is a sox effect) are not available, so this build restates them (DESIGN.md §4 "augment", parity UNPINNED
against the real libraries), and they are used only when the environment variable SPARCH_AUGMENT is "restated" when
the dataset is constructed.  Unset or empty, `use_augm=True` raises NotImplementedError as before: training without
augmentation, or with a different one, while the caller asked for the reference's would be worse.  Any other value
is a ValueError.  With the variable set, the HD `train` and SC `training` splits draw the reference's per-clip
decisions once per batch in the collate function (`augment.draw_augmentation`: Python's `random` and torch's
generator in the reference's order) and apply them to the decoded batch on the device (`functional.augment_padded`)
before the features; the other splits are not augmented, as in the reference.  The first-batch MD5 check reads the
decoded samples before augmentation.

SPARCH_AUDIO=resident (or `load_hd_or_sc(..., resident="resident")`) keeps the whole split on the device instead
(`functional.AudioStore`): the clips are read (FLAC: decoded on the device) and uploaded once, and every batch is
built there from the list of its clip indices — one kernel (`sparch_audio_gather_fbank`), two for an augmented split
(`sparch_audio_gather_augment`, then the padded fbank).  The index lists come from a torch DataLoader built with the
arguments of the file loader and the augmentation draws are made per batch where the collate function makes them,
so with equal seeds the batches are the file loader's bit for bit.  The samples come from the pack file
`{data_folder}/{dataset}_{split}.audio.npz` when it exists (tools/pack_audio.py), else from the files.
"""
import logging
import os
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from ..functional import AudioStore, augment_padded, fbank_padded, flac_decode_padded, flac_error_message
from ._index import _index_loader, _SampleIndices
from .audio import FlacError, FlacStream, flac_md5_ok, read_clip
from .augment import draw_augmentation

logger = logging.getLogger(__name__)

SAMPLE_RATE = 16000
EXCEPT_FOLDER = "_background_noise_"


def hd_label(filename):
    """Digit in the last character of the file stem, plus 10 for German (nonspiking_datasets.py:98-100 reads
    name[-6], which assumes a five-character extension such as ".flac")."""
    name = os.path.basename(filename)
    return int(os.path.splitext(name)[0][-1]) + (10 if name[5] == "g" else 0)


AUGMENT_ENV = "SPARCH_AUGMENT"


def _augmentation(use_augm, augmented_split, min_snr, max_snr, p_noise):
    """(min_snr, max_snr, p_noise) when this split is augmented, else None.  use_augm needs SPARCH_AUGMENT=restated,
    read here (at construction) and not at import."""
    if not use_augm:
        return None
    mode = os.environ.get(AUGMENT_ENV, "")
    if mode == "":
        raise NotImplementedError("sparch_amd.dataloaders: data augmentation of HD / SC (torchaudio_augmentations "
                                  "in the reference) is not part of this build; run with --use_augm False. "
                                  f"{AUGMENT_ENV}=restated selects this build's restatement of it (unpinned).")
    if mode != "restated":
        raise ValueError(f"{AUGMENT_ENV}={mode!r}: the only value is 'restated'")
    return (min_snr, max_snr, p_noise) if augmented_split else None


class _AudioClips(Dataset):
    """Clips `file_list` with class indices `targets`; host decoding of WAV per item, FLAC decoding and features per
    batch on the device."""

    def __init__(self, file_list, targets, device, augment=None):
        self.file_list, self.targets, self.device = file_list, targets, device
        self.augment = augment  # (min_snr, max_snr, p_noise) of an augmented split, else None
        self._rate_warned = False
        self._md5_checked = False
        self._pending = []  # (event, pinned error record, file names) of batches whose FLAC errors are unread

    def __len__(self):
        return len(self.file_list)

    def __getitem__(self, index):
        """(clip, label): the samples of channel 0 on the host for WAV (int16 for 16-bit mono PCM, float32
        otherwise), an audio.FlacStream (file bytes and STREAMINFO, not decoded) for FLAC."""
        x, rate = read_clip(self.file_list[index])
        if rate != SAMPLE_RATE and not self._rate_warned:
            self._rate_warned = True
            logger.warning(f"{self.file_list[index]}: sample rate {rate} Hz; the features assume {SAMPLE_RATE} Hz "
                           "and nothing is resampled (as in the reference). Warned once per dataset.")
        return x, self.targets[index]

    def generateBatch(self, batch):
        """(xs (B, T_max, 40) on the device, xlens (B,) frame counts, ys (B,)): nonspiking_datasets.py:104-111 with
        the features made once per batch on the device."""
        self.check_decode_errors(wait=False)
        clips, ys = zip(*batch)
        flac = [i for i, c in enumerate(clips) if isinstance(c, FlacStream)]
        lengths = [c.info.total_samples if isinstance(c, FlacStream) else len(c) for c in clips]
        pcm16 = all(c.info.bps == 16 and c.info.channels == 1 if isinstance(c, FlacStream) else c.dtype == np.int16
                    for c in clips)
        # a fresh pinned buffer per batch: the caching host allocator does not hand it out again before the
        # non-blocking copy from it has completed, and nothing writes to it after the copy is enqueued
        host = torch.empty(len(clips), max(lengths), dtype=torch.int16 if pcm16 else torch.float32,
                           pin_memory=torch.cuda.is_available())
        rows = host.numpy()
        for row, c, n in zip(rows, clips, lengths):  # the kernel reads no sample past a clip's length
            if not isinstance(c, FlacStream):
                row[:n] = c if pcm16 or c.dtype == np.float32 else c.astype(np.float32) / np.float32(2 ** 15)
        wave = host.to(self.device, non_blocking=True)
        if flac:  # FLAC rows: decoded on the device into the same buffer (their host rows are not read)
            streams = [clips[i] for i in flac]
            err = flac_decode_padded([c.data for c in streams], [c.info for c in streams], wave, rows=flac)
            names = [c.path for c in streams]
            if not self._md5_checked:
                self._md5_checked = True
                self._check_md5(wave, flac, streams, err)
            else:
                rec = torch.empty(2, dtype=torch.int64, pin_memory=True)
                rec.copy_(err, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                self._pending.append((ev, rec, names))
        if self.augment is not None:  # nonspiking_datasets.py:93, 191, per clip in batch order; sox is told 16 kHz
            min_snr, max_snr, p_noise = self.augment
            params, noise_seed = draw_augmentation(len(clips), min_snr, max_snr, p_noise)
            wave = augment_padded(wave, lengths, params, noise_seed, min_snr, max_snr, sample_rate=SAMPLE_RATE)
        xs, xlens = fbank_padded(wave, lengths, num_mel_bins=40)
        return xs, xlens, torch.LongTensor(ys)

    def _check_md5(self, wave, flac, streams, err):
        """First FLAC batch of the dataset: decode errors, then the MD5 of every mono clip that carries one."""
        msg = flac_error_message(err.cpu(), [c.path for c in streams])
        if msg:
            raise FlacError(msg)
        mono = [(i, c) for i, c in zip(flac, streams) if c.info.channels == 1 and c.info.md5 != bytes(16)]
        if mono:
            rows = wave[[i for i, _ in mono]].cpu().numpy()
            for row, (_, c) in zip(rows, mono):
                if not flac_md5_ok(row[:c.info.total_samples], c.info):
                    raise FlacError(f"{c.path}: decoded samples do not match the STREAMINFO MD5")

    def check_decode_errors(self, wait=True):
        """Raise FlacError for the first failed FLAC file of the batches collated so far whose decoding has completed
        (wait=True: of all of them, waiting for the device)."""
        while self._pending:
            ev, rec, names = self._pending[0]
            if wait:
                ev.synchronize()
            elif not ev.query():
                return
            self._pending.pop(0)
            msg = flac_error_message(rec, names)
            if msg:
                self._pending.clear()
                raise FlacError(msg)


class _EpochCheckedLoader(DataLoader):
    """A DataLoader whose iteration ends by reading the decode error records of the epoch's last batches."""

    def __iter__(self):
        yield from super().__iter__()
        self.dataset.check_decode_errors(wait=True)


class HeidelbergDigits(_AudioClips):
    """nonspiking_datasets.py:31-111.  Files: `<data_folder>/<split>_filenames.txt`, audio under
    `<data_folder>/audio/`."""

    def __init__(self, data_folder, split, use_augm, min_snr, max_snr, p_noise, device="cuda"):
        if split not in ["train", "test"]:
            raise ValueError(f"Invalid split {split}")
        augment = _augmentation(use_augm, split == "train", min_snr, max_snr, p_noise)
        self.data_folder = data_folder
        with open(os.path.join(data_folder, f"{split}_filenames.txt")) as f:
            names = [n for n in f.read().splitlines() if n.strip()]
        super().__init__([os.path.join(data_folder, "audio", n) for n in names], [hd_label(n) for n in names],
                         device, augment)


class SpeechCommands(_AudioClips):
    """nonspiking_datasets.py:115-209.  `training`: every */*.wav under `data_folder`, sorted, minus the files of
    validation_list.txt and testing_list.txt and anything under _background_noise_; `validation` / `testing`: the
    files of the list, in list order.  Label: index of the file's folder in `labels`."""

    def __init__(self, data_folder, split, use_augm, min_snr, max_snr, p_noise, device="cuda"):
        if split not in ["training", "validation", "testing"]:
            raise ValueError(f"Invalid split {split}")
        augment = _augmentation(use_augm, split == "training", min_snr, max_snr, p_noise)
        self.data_folder = data_folder

        def load_list(filename):  # paths relative to data_folder, normalised ("./yes/a.wav" -> "yes/a.wav")
            with open(os.path.join(data_folder, filename)) as f:
                return [os.path.normpath(line.strip()) for line in f if line.strip()]

        if split == "training":
            exclude = set(load_list("validation_list.txt") + load_list("testing_list.txt"))
            files = sorted(os.path.relpath(p, data_folder) for p in Path(data_folder).glob("*/*.wav"))
            files = [w for w in files if w not in exclude and EXCEPT_FOLDER not in w]
        else:
            files = load_list(f"{split}_list.txt")
        self.labels = sorted(next(os.walk(data_folder))[1])[1:]
        super().__init__([os.path.join(data_folder, w) for w in files],
                         [self.labels.index(os.path.dirname(w)) for w in files], device, augment)


class ResidentAudioLoader:
    """Batches `(xs, xlens, ys)` of an `AudioStore`: xs and ys on the device, xlens on the host as the file loader
    gives them.  Iterating draws the epoch's index lists from a DataLoader over the clip numbers (so `len`, the short
    last batch, `.sampler` / `set_epoch` and the global generator behave as with the file loader), uploads them in
    one copy, and per batch makes the augmentation draws of an augmented split (`augment`: (min_snr, max_snr,
    p_noise), else None) where the file loader's collate makes them, then launches the kernel(s)."""

    def __init__(self, store, batch_size, shuffle=True, rank=0, world=1, seed=0, augment=None):
        self.store, self.batch_size, self.augment = store, batch_size, augment
        self.index_loader = _index_loader(_SampleIndices(len(store)), batch_size, shuffle, rank, world, seed)
        self.sampler = self.index_loader.sampler

    def __len__(self):
        return len(self.index_loader)

    def index_lists(self):
        """The clip indices of every batch of one epoch (host tensors), in order."""
        return [b.to(torch.int64) for b in self.index_loader]

    def draw(self, n_clips):
        """The augmentation of one batch, (params, noise_seed, min_snr, max_snr), or None for a plain split."""
        if self.augment is None:
            return None
        min_snr, max_snr, p_noise = self.augment
        params, noise_seed = draw_augmentation(n_clips, min_snr, max_snr, p_noise)
        return params, noise_seed, min_snr, max_snr

    def __iter__(self):
        lists = self.index_lists()
        if not lists:
            return
        flat = torch.cat(lists).to(self.store.device)
        at = 0
        for b in lists:
            n = b.numel()
            yield self.store.batch(flat[at:at + n], b, augment=self.draw(n), sample_rate=SAMPLE_RATE)
            at += n


def _audio_pack_path(data_folder, dataset_name, split):
    return f"{data_folder}/{dataset_name}_{split}.audio.npz"


def _dataset(dataset_name, data_folder, split, use_augm=False, min_snr=0.0001, max_snr=0.9, p_noise=0.1,
             device="cuda"):
    """(dataset, the split's own name): the clips of `split` ("train" / "valid" / "test") of "hd" or "sc"."""
    if dataset_name == "hd":
        if split in ["valid", "test"]:
            split = "test"
            logging.info("\nHD uses the same split for validation and testing.\n")
        return HeidelbergDigits(data_folder, split, use_augm, min_snr, max_snr, p_noise, device=device), split
    split = {"train": "training", "valid": "validation", "test": "testing"}[split]
    return SpeechCommands(data_folder, split, use_augm, min_snr, max_snr, p_noise, device=device), split


def load_hd_or_sc(dataset_name, data_folder, split, batch_size, shuffle=True, use_augm=False, min_snr=0.0001,
                  max_snr=0.9, p_noise=0.1, workers=0, device="cuda", rank=0, world=1, seed=0, resident=None):
    """nonspiking_datasets.py:212-290.  rank / world (data-parallel runs; not in the reference): every rank lists
    the same files and draws a disjoint 1/world share of each epoch's (shuffled) order through a
    DistributedSampler — call `loader.sampler.set_epoch(e)` per epoch; `batch_size` is the PER-RANK batch.
    resident: None reads SPARCH_AUDIO; unset or empty = the file loader, "resident" = a `ResidentAudioLoader` (every
    rank keeps the whole split on its device); anything else is a ValueError."""
    if resident is None:
        resident = os.environ.get("SPARCH_AUDIO", "")
    if resident not in ("", "resident"):
        raise ValueError(f"SPARCH_AUDIO / resident: unknown value '{resident}' (unset or empty: file loader; "
                         "'resident': the split's clips stay on the device)")
    if dataset_name not in ["hd", "sc"]:
        raise ValueError(f"Invalid dataset name {dataset_name}")
    if split not in ["train", "valid", "test"]:
        raise ValueError(f"Invalid split name {split}")
    if workers != 0:
        raise ValueError("sparch_amd.dataloaders: the collate function computes the features on the GPU; use "
                         "workers=0 (the reference's default)")
    dataset, split = _dataset(dataset_name, data_folder, split, use_augm, min_snr, max_snr, p_noise, device)
    logging.info(f"Number of examples in {dataset_name} {split} set: {len(dataset)}")
    if resident == "resident":
        pack = _audio_pack_path(data_folder, dataset_name, split)
        if os.path.exists(pack):
            store = AudioStore.from_pack(pack, device=device)
            if len(store) != len(dataset):
                raise ValueError(f"{pack}: {len(store)} clips, the {split} set lists {len(dataset)}; write the pack "
                                 "again (tools/pack_audio.py)")
        else:
            store = AudioStore.from_files(dataset.file_list, dataset.targets, device=device, sample_rate=SAMPLE_RATE)
        logging.info(f"Clips of the {dataset_name} {split} set are resident on {store.device}: {len(store)} clips, "
                     f"{store.nbytes / 2**20:.1f} MiB, {'int16' if store.int16 else 'fp32'} samples, from the "
                     f"{'pack ' + pack if store.source == 'pack' else 'files'}"
                     f"{', augmented per batch on the device' if dataset.augment is not None else ''}")
        return ResidentAudioLoader(store, batch_size, shuffle, rank, world, seed, augment=dataset.augment)
    if world > 1:
        from torch.utils.data.distributed import DistributedSampler

        sampler = DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=shuffle, seed=seed)
        return _EpochCheckedLoader(dataset, batch_size=batch_size, collate_fn=dataset.generateBatch,
                                   sampler=sampler, num_workers=0, pin_memory=False)
    return _EpochCheckedLoader(dataset, batch_size=batch_size, collate_fn=dataset.generateBatch, shuffle=shuffle,
                               num_workers=0, pin_memory=False)
