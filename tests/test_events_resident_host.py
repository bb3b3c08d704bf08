"""CPU: the host side of the resident SHD / SSC event store (SPARCH_EVENTS=resident) — the pack file, the
option's parsing, and the index lists of the resident loader against the sample order of the per-sample loader."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from sparch_amd import functional as Fn
from sparch_amd.dataloaders import spiking_datasets as sd
from tests.event_cases import fake_h5

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.parametrize("tdtype", [np.float16, np.float32])
def test_pack_round_trip(tmp_path, tdtype):
    import pack_events

    h5 = fake_h5(tdtype=tdtype)
    path = str(tmp_path / "shd_train.events.npz")
    pack_events.pack_mapping(h5, path)
    a = Fn.load_event_pack(path)
    assert a["times"].dtype == tdtype and a["units"].dtype == np.uint16
    assert a["offsets"].dtype == np.int64 and a["labels"].dtype == np.int64
    np.testing.assert_array_equal(a["labels"], np.asarray(h5["labels"], np.int64))
    assert len(a["offsets"]) == 12 and a["offsets"][0] == 0 and a["offsets"][-1] == len(a["times"])
    for i in range(11):
        lo, hi = a["offsets"][i], a["offsets"][i + 1]
        np.testing.assert_array_equal(a["times"][lo:hi], h5["spikes"]["times"][i])   # bit for bit, same dtype
        np.testing.assert_array_equal(a["units"][lo:hi], h5["spikes"]["units"][i])
    assert a["offsets"][5] == a["offsets"][4]                                          # the empty sample
    # uncompressed: the arrays are stored, not deflated
    import zipfile
    with zipfile.ZipFile(path) as z:
        assert all(i.compress_type == zipfile.ZIP_STORED for i in z.infolist())


def test_pack_conversions():
    """float64 times are rounded to float32 (what SpikingDataset.__getitem__ does); a unit that is negative or does
    not fit 16 bits is stored as 0xFFFF; mixed float16 / float32 rows give float32."""
    h5 = {"spikes": {"times": [np.array([0.1, 0.7], np.float64), np.array([0.5], np.float64)],
                     "units": [np.array([-3, 70000], np.int64), np.array([699], np.int64)]},
          "labels": [1, 2]}
    a = Fn.event_arrays_from_mapping(h5)
    assert a["times"].dtype == np.float32
    np.testing.assert_array_equal(a["times"], np.array([0.1, 0.7, 0.5], np.float64).astype(np.float32))
    np.testing.assert_array_equal(a["units"], np.array([0xFFFF, 0xFFFF, 699], np.uint16))
    h5["spikes"]["times"] = [np.array([0.1, 0.7], np.float16), np.array([0.5], np.float32)]
    assert Fn.event_arrays_from_mapping(h5)["times"].dtype == np.float32
    assert Fn._samples_sorted(a["times"], a["offsets"])              # 0.7 -> 0.5 straddles two samples
    assert not Fn._samples_sorted(np.array([0.2, 0.1, 0.5], np.float32), np.array([0, 2, 3]))
    assert not Fn._samples_sorted(np.array([0.1, np.nan, 0.5], np.float32), np.array([0, 3]))


def test_malformed_packs_raise(tmp_path):
    good = Fn.event_arrays_from_mapping(fake_h5())

    def written(**change):
        a = dict(good)
        a.update(change)
        path = str(tmp_path / f"bad{len(os.listdir(tmp_path))}.npz")
        with open(path, "wb") as f:
            np.savez(f, **{k: v for k, v in a.items() if v is not None})
        return path

    Fn.load_event_pack(written())                                       # the unchanged arrays load
    off = good["offsets"].copy()
    off[3], off[4] = off[4] + 1, off[3]
    dec = good["offsets"].copy()
    dec[2] = dec[3] + 1
    for bad in (dict(offsets=dec),                                      # offsets decreasing
                dict(offsets=good["offsets"] + 1),                      # does not start at 0 / last != n_events
                dict(times=good["times"][:-1]),                         # last offset is not the number of events
                dict(units=good["units"][:-1]),
                dict(labels=good["labels"][:-1]),                       # label count
                dict(units=good["units"].astype(np.int32)),             # wrong dtype
                dict(times=good["times"].astype(np.float64)),
                dict(labels=None)):                                     # an array missing
        with pytest.raises(ValueError):
            Fn.load_event_pack(written(**bad))
    with pytest.raises(ValueError):
        Fn.save_event_pack(str(tmp_path / "never.npz"), dict(good, offsets=dec))
    assert not os.path.exists(tmp_path / "never.npz")


def test_store_that_does_not_fit_is_refused():
    with pytest.raises(RuntimeError, match="free"):
        Fn._require_room(10 * 2**20, 4 * 2**20, "EventStore")
    Fn._require_room(4 * 2**20, 4 * 2**20, "EventStore")


def test_option_parsing(monkeypatch):
    monkeypatch.setenv("SPARCH_EVENTS", "bogus")
    with pytest.raises(ValueError, match="SPARCH_EVENTS"):
        sd.load_shd_or_ssc("shd", "/unused", "train", 4, h5_file=fake_h5(), device="cpu")
    with pytest.raises(ValueError):
        sd.load_shd_or_ssc("shd", "/unused", "train", 4, h5_file=fake_h5(), device="cpu", resident="yes")
    for value in (None, ""):
        if value is None:
            monkeypatch.delenv("SPARCH_EVENTS")
        else:
            monkeypatch.setenv("SPARCH_EVENTS", value)
        loader = sd.load_shd_or_ssc("shd", "/unused", "train", 4, h5_file=fake_h5(), device="cpu")
        assert type(loader) is torch.utils.data.DataLoader and isinstance(loader.dataset, sd.SpikingDataset)
    # an explicit argument wins over the environment
    monkeypatch.setenv("SPARCH_EVENTS", "resident")
    loader = sd.load_shd_or_ssc("shd", "/unused", "train", 4, h5_file=fake_h5(), device="cpu", resident="")
    assert type(loader) is torch.utils.data.DataLoader


def test_resident_mode_without_pack_or_h5py_names_the_package(tmp_path):
    try:
        import h5py  # noqa: F401
        pytest.skip("h5py is installed: the .h5 path would be taken")
    except ImportError:
        pass
    with pytest.raises(ImportError, match="h5py"):
        sd.load_shd_or_ssc("shd", str(tmp_path), "train", 4, resident="resident", device="cpu")


class _HostStore:
    """Stands in for an EventStore on a machine without a GPU: the index lists need its length only."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def prepare(self, nb_steps):
        return 1


class _Recorder(sd.SpikingDataset):
    """The per-sample loader's dataset, recording which samples each batch asked for."""

    def generateBatch(self, batch):
        return [int(lbl) for _, _, lbl in batch]


def _orders(n, batch_size, shuffle, rank, world, seed, epochs=2):
    """Per epoch: (sample order of the per-sample loader, index lists of the resident loader, generator states)."""
    h5 = fake_h5(n=n)
    h5["labels"] = np.arange(n)                                  # the label of a sample is its number
    out = []
    for which in ("today", "resident"):
        torch.manual_seed(99)
        if which == "today":
            ds = _Recorder("shd", "/unused", "train", h5_file=h5, device="cpu")
            loader = sd._index_loader(ds, batch_size, shuffle, rank, world, seed, collate_fn=ds.generateBatch)
            real = sd.load_shd_or_ssc("shd", "/unused", "train", batch_size, shuffle=shuffle, h5_file=h5, device="cpu",
                                      rank=rank, world=world, seed=seed, resident="")
            assert type(real.sampler) is type(loader.sampler) and real.batch_size == loader.batch_size
        else:
            loader = sd.ResidentEventLoader(_HostStore(n), batch_size, 100, shuffle, rank, world, seed)
        got = []
        for e in range(epochs):
            if world > 1:
                loader.sampler.set_epoch(e)
            if which == "today":
                lists = [list(b) for b in loader]
            else:
                lists = [b.tolist() for b in loader.index_lists()]
            got.append((lists, torch.get_rng_state().clone()))
        assert len(loader) == len(got[0][0])
        out.append(got)
    return out


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
def test_index_lists_equal_the_per_sample_loaders_order(shuffle, rank, world):
    today, resident = _orders(n=21, batch_size=4, shuffle=shuffle, rank=rank, world=world, seed=5)
    for (lists_t, rng_t), (lists_r, rng_r) in zip(today, resident):
        assert lists_t == lists_r
        assert len(lists_r[-1]) < 4                               # the short last batch is there
        assert torch.equal(rng_t, rng_r), "torch's global generator differs after the epoch"
    if shuffle:
        assert today[0][0] != today[1][0]                         # a fresh permutation per epoch
    if world == 2:
        assert sum(len(b) for b in resident[0][0]) == 11          # 21 samples padded to 22, half each


def test_pack_events_cli_without_files(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pack_events.py"), "--data_folder", str(tmp_path),
                        "--dataset_name", "shd"], capture_output=True, text=True)
    assert r.returncode != 0 and "no shd_" in (r.stderr + r.stdout)
