"""
HD / SC loader with the reference's API (sparch/dataloaders/nonspiking_datasets.py):
`HeidelbergDigits(data_folder, split, use_augm, min_snr, max_snr, p_noise)`,
`SpeechCommands(data_folder, split, use_augm, min_snr, max_snr, p_noise)` and
`load_hd_or_sc(dataset_name, data_folder, split, batch_size, shuffle=True, use_augm=False, min_snr=0.0001,
max_snr=0.9, p_noise=0.1, workers=0)`, whose batches keep the `(xs, xlens, ys)` collate contract
(nonspiking_datasets.py:104-111, 202-209): xs (B, T_max, 40) log-mel features, padded with zeros after each
clip's own frames, xlens the frame counts, ys a LongTensor.

What differs is WHERE the features are made: the reference runs torchaudio's kaldi.fbank per clip on the CPU in
`__getitem__` and pads in the collate function; here `__getitem__` returns the decoded host samples of a clip
(`audio.read_audio`), and the collate function packs the batch into one pinned buffer, uploads it (16-bit PCM as
int16) and makes the padded features with one kernel (`functional.fbank_padded`).

File lists, their order and the labels are the reference's, with two of its bugs left out:
  * SC labels are the sorted subdirectories of `data_folder` minus the first (`_background_noise_` in the v0.02
    layout); the reference lists them with `os.walk("./" + data_folder)`, which breaks absolute paths;
  * the SC training split drops the files named in validation_list.txt and testing_list.txt; the reference
    compares path strings, which silently drops nothing when `data_folder` starts with "./".  Here paths are
    compared relative to `data_folder`.
`use_augm=True` raises NotImplementedError: the reference's augmentation (torchaudio_augmentations, whose Reverb
is a sox effect) is not available, and training without it while the caller asked for it would be worse.
"""
import logging
import os
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from ..functional import fbank_padded
from .audio import read_audio

logger = logging.getLogger(__name__)

SAMPLE_RATE = 16000
EXCEPT_FOLDER = "_background_noise_"


def hd_label(filename):
    """Digit in the last character of the file stem, plus 10 for German (nonspiking_datasets.py:98-100 reads
    name[-6], which assumes a five-character extension such as ".flac")."""
    name = os.path.basename(filename)
    return int(os.path.splitext(name)[0][-1]) + (10 if name[5] == "g" else 0)


def _refuse_augmentation(use_augm):
    if use_augm:
        raise NotImplementedError("sparch_amd.dataloaders: data augmentation of HD / SC (torchaudio_augmentations "
                                  "in the reference) is not part of this build; run with --use_augm False")


class _AudioClips(Dataset):
    """Clips `file_list` with class indices `targets`; host decoding per item, features per batch on the device."""

    def __init__(self, file_list, targets, device):
        self.file_list, self.targets, self.device = file_list, targets, device
        self._rate_warned = False

    def __len__(self):
        return len(self.file_list)

    def __getitem__(self, index):
        """(samples of channel 0 on the host: int16 for 16-bit mono PCM, float32 otherwise; label)."""
        x, rate = read_audio(self.file_list[index])
        if rate != SAMPLE_RATE and not self._rate_warned:
            self._rate_warned = True
            logger.warning(f"{self.file_list[index]}: sample rate {rate} Hz; the features assume {SAMPLE_RATE} Hz "
                           "and nothing is resampled (as in the reference). Warned once per dataset.")
        return x, self.targets[index]

    def generateBatch(self, batch):
        """(xs (B, T_max, 40) on the device, xlens (B,) frame counts, ys (B,)): nonspiking_datasets.py:104-111 with
        the features made once per batch on the device."""
        clips, ys = zip(*batch)
        lengths = [len(c) for c in clips]
        pcm16 = all(c.dtype == np.int16 for c in clips)
        # a fresh pinned buffer per batch: the caching host allocator does not hand it out again before the
        # non-blocking copy from it has completed, and nothing writes to it after the copy is enqueued
        host = torch.empty(len(clips), max(lengths), dtype=torch.int16 if pcm16 else torch.float32,
                           pin_memory=torch.cuda.is_available())
        rows = host.numpy()
        for row, c, n in zip(rows, clips, lengths):  # the kernel reads no sample past a clip's length
            row[:n] = c if pcm16 or c.dtype == np.float32 else c.astype(np.float32) / np.float32(2 ** 15)
        wave = host.to(self.device, non_blocking=True)
        xs, xlens = fbank_padded(wave, lengths, num_mel_bins=40)
        return xs, xlens, torch.LongTensor(ys)


class HeidelbergDigits(_AudioClips):
    """nonspiking_datasets.py:31-111.  Files: `<data_folder>/<split>_filenames.txt`, audio under
    `<data_folder>/audio/`."""

    def __init__(self, data_folder, split, use_augm, min_snr, max_snr, p_noise, device="cuda"):
        if split not in ["train", "test"]:
            raise ValueError(f"Invalid split {split}")
        _refuse_augmentation(use_augm)
        self.data_folder = data_folder
        with open(os.path.join(data_folder, f"{split}_filenames.txt")) as f:
            names = [n for n in f.read().splitlines() if n.strip()]
        super().__init__([os.path.join(data_folder, "audio", n) for n in names], [hd_label(n) for n in names],
                         device)


class SpeechCommands(_AudioClips):
    """nonspiking_datasets.py:115-209.  `training`: every */*.wav under `data_folder`, sorted, minus the files of
    validation_list.txt and testing_list.txt and anything under _background_noise_; `validation` / `testing`: the
    files of the list, in list order.  Label: index of the file's folder in `labels`."""

    def __init__(self, data_folder, split, use_augm, min_snr, max_snr, p_noise, device="cuda"):
        if split not in ["training", "validation", "testing"]:
            raise ValueError(f"Invalid split {split}")
        _refuse_augmentation(use_augm)
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
                         [self.labels.index(os.path.dirname(w)) for w in files], device)


def load_hd_or_sc(dataset_name, data_folder, split, batch_size, shuffle=True, use_augm=False, min_snr=0.0001,
                  max_snr=0.9, p_noise=0.1, workers=0, device="cuda", rank=0, world=1, seed=0):
    """nonspiking_datasets.py:212-290.  rank / world (data-parallel runs; not in the reference): every rank lists
    the same files and draws a disjoint 1/world share of each epoch's (shuffled) order through a
    DistributedSampler — call `loader.sampler.set_epoch(e)` per epoch; `batch_size` is the PER-RANK batch."""
    if dataset_name not in ["hd", "sc"]:
        raise ValueError(f"Invalid dataset name {dataset_name}")
    if split not in ["train", "valid", "test"]:
        raise ValueError(f"Invalid split name {split}")
    if workers != 0:
        raise ValueError("sparch_amd.dataloaders: the collate function computes the features on the GPU; use "
                         "workers=0 (the reference's default)")
    if dataset_name == "hd":
        if split in ["valid", "test"]:
            split = "test"
            logging.info("\nHD uses the same split for validation and testing.\n")
        dataset = HeidelbergDigits(data_folder, split, use_augm, min_snr, max_snr, p_noise, device=device)
    else:
        split = {"train": "training", "valid": "validation", "test": "testing"}[split]
        dataset = SpeechCommands(data_folder, split, use_augm, min_snr, max_snr, p_noise, device=device)
    logging.info(f"Number of examples in {dataset_name} {split} set: {len(dataset)}")
    if world > 1:
        from torch.utils.data.distributed import DistributedSampler

        sampler = DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=shuffle, seed=seed)
        return DataLoader(dataset, batch_size=batch_size, collate_fn=dataset.generateBatch, sampler=sampler,
                          num_workers=0, pin_memory=False)
    return DataLoader(dataset, batch_size=batch_size, collate_fn=dataset.generateBatch, shuffle=shuffle,
                      num_workers=0, pin_memory=False)
