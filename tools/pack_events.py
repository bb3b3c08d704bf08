#!/usr/bin/env python
"""Write the event pack of an SHD / SSC split: `{data_folder}/{dataset}_{split}.events.npz`, an uncompressed
np.savez of the four flat arrays of `sparch_amd.functional.EventStore` (times float16 / float32 as the file has
them, units uint16, offsets int64, labels int64).  With SPARCH_EVENTS=resident the loader reads the pack instead
of the .h5 file, so a machine without h5py can train on packs made where h5py exists:

    python tools/pack_events.py --data_folder data/shd --dataset_name shd            # every split it finds

`pack_mapping(mapping, path)` does the same for anything laid out like the file (tests, synthetic stores).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPLITS = {"shd": ("train", "test"), "ssc": ("train", "valid", "test")}


def pack_mapping(mapping, path):
    from sparch_amd.functional import event_arrays_from_mapping, save_event_pack

    arrays = event_arrays_from_mapping(mapping)
    save_event_pack(path, arrays)
    return arrays


def pack_split(data_folder, dataset_name, split):
    from sparch_amd.dataloaders.spiking_datasets import _event_pack_path, _open_h5

    with _open_h5(f"{data_folder}/{dataset_name}_{split}.h5") as f:
        path = _event_pack_path(data_folder, dataset_name, split)
        arrays = pack_mapping(f, path)
    return path, arrays


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data_folder", required=True)
    ap.add_argument("--dataset_name", required=True, choices=sorted(SPLITS))
    ap.add_argument("--splits", nargs="*", default=None, help="default: every split whose .h5 file exists")
    a = ap.parse_args()
    splits = a.splits or [s for s in SPLITS[a.dataset_name]
                          if os.path.exists(f"{a.data_folder}/{a.dataset_name}_{s}.h5")]
    if not splits:
        sys.exit(f"no {a.dataset_name}_*.h5 file in {a.data_folder}")
    for split in splits:
        path, arrays = pack_split(a.data_folder, a.dataset_name, split)
        print(f"{path}: {len(arrays['labels'])} samples, {len(arrays['times'])} events, times "
              f"{arrays['times'].dtype}, {os.path.getsize(path) / 2**20:.1f} MiB")


if __name__ == "__main__":
    main()
