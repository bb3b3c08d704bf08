#!/usr/bin/env python
"""Write the audio packs of Heidelberg Digits or Speech Commands: `{data_folder}/{dataset}_{split}.audio.npz` for
every split (hd: train, test; sc: training, validation, testing), an uncompressed np.savez of the four flat arrays
of `sparch_amd.functional.AudioStore` (samples int16 when every clip of the split is 16-bit mono, else float32;
starts int64, lengths int32, labels int64).  With SPARCH_AUDIO=resident the loader reads the pack instead of the
split's files:

    python tools/pack_audio.py data/speech_commands sc

The file lists, their order and the labels are those of the loader's own `HeidelbergDigits` / `SpeechCommands`.  A
tree of WAV files is packed on any host.  FLAC clips are decoded on the device (this build has no host FLAC
decoder): a tree that holds some needs a HIP device, and the tool says so when none is visible.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPLITS = {"hd": ("train", "test"), "sc": ("train", "valid", "test")}  # load_hd_or_sc's names


def pack_split(data_folder, dataset_name, split, device="cuda"):
    """(path, arrays) of one split, written.  The device is asked for only when the split holds FLAC clips."""
    from sparch_amd.dataloaders.nonspiking_datasets import SAMPLE_RATE, _audio_pack_path, _dataset
    from sparch_amd.functional import audio_arrays_from_files, save_audio_pack

    dataset, own_name = _dataset(dataset_name, data_folder, split, device=device)
    arrays = audio_arrays_from_files(dataset.file_list, dataset.targets, device=device, sample_rate=SAMPLE_RATE)
    path = _audio_pack_path(data_folder, dataset_name, own_name)
    save_audio_pack(path, arrays)
    return path, arrays


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("data_folder")
    ap.add_argument("dataset_name", choices=sorted(SPLITS))
    a = ap.parse_args(argv)
    for split in SPLITS[a.dataset_name]:
        try:
            path, arrays = pack_split(a.data_folder, a.dataset_name, split)
        except RuntimeError as e:
            if "no HIP device" in str(e):
                sys.exit(f"pack_audio: {e}")
            raise
        print(f"{path}: {len(arrays['labels'])} clips, {len(arrays['samples'])} samples, "
              f"{arrays['samples'].dtype}, {os.path.getsize(path) / 2**20:.1f} MiB")


if __name__ == "__main__":
    main()
