"""CPU: the host side of the resident HD / SC audio store (SPARCH_AUDIO=resident) — the array checks, the pack file
and tools/pack_audio.py, the int16 / fp32 decision, the option's parsing, the argument checks of the two new entry
points (no launch), and the index lists and augmentation draws of the resident loader against a loader that draws
inside its collate function."""
import os
import random
import re
import sys
import zipfile

import numpy as np
import pytest
import torch

from sparch_amd import _capi
from sparch_amd import functional as Fn
from sparch_amd.dataloaders import _index
from sparch_amd.dataloaders import nonspiking_datasets as nd
from sparch_amd.dataloaders import spiking_datasets as sd
from sparch_amd.dataloaders.audio import read_clip
from sparch_amd.dataloaders.augment import draw_augmentation
from tests import flac_writer as fw
from tests.audio_trees import make_hd_tree, make_sc_tree, write_pcm_wav

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LENGTHS = (16000, 9000, 401, 12345)


def good_arrays(dtype=np.int16):
    g = np.random.default_rng(0)
    lengths = np.array([500, 0, 401, 1000], np.int32)
    starts = np.array([3, 503, 503, 1000], np.int64)           # gaps are allowed; the empty clip sits on a boundary
    x = g.integers(-2000, 2000, 2100).astype(dtype) if dtype == np.int16 else g.uniform(-1, 1, 2100).astype(dtype)
    return {"samples": x, "starts": starts, "lengths": lengths, "labels": np.array([4, 5, 6, 7], np.int64)}


# ----------------------------------------------------------------------------------------- arrays and packs
def test_array_checks_refuse_each_malformed_store_by_name():
    good = good_arrays()
    out = Fn.check_audio_arrays(good)
    assert sorted(out) == sorted(Fn.AUDIO_PACK_KEYS) and all(out[k] is good[k] for k in good)
    Fn.check_audio_arrays(good_arrays(np.float32))
    s, n = good["starts"], good["lengths"]

    def changed(key, at, value):
        v = good[key].copy()
        v[at] = value
        return dict(good, **{key: v})

    for bad, words in ((changed("starts", 0, -1), "clip 0 has a negative start"),
                       (changed("lengths", 3, 1101), "clip 3 ends at sample 2101, past the end of samples"),
                       (changed("starts", 3, 2000), "clip 3 ends at sample 3000, past the end"),
                       (changed("starts", 2, 400), "clips 2 and 0 overlap|clips 0 and 2 overlap"),
                       (changed("lengths", 2, 498), "clips 2 and 3 overlap"),
                       (changed("lengths", 1, -5), "clip 1 has a negative length"),
                       (dict(good, labels=good["labels"][:-1]), "must have one length, found 4, 4, 3"),
                       (dict(good, starts=s[:-1]), "must have one length, found 3, 4, 4"),
                       (dict(good, lengths=n[:-1]), "must have one length, found 4, 3, 4"),
                       (dict(good, samples=good["samples"].astype(np.int32)), "dtypes must be"),
                       (dict(good, samples=good["samples"].astype(np.float64)), "dtypes must be"),
                       (dict(good, starts=s.astype(np.int32)), "dtypes must be"),
                       (dict(good, lengths=n.astype(np.int64)), "dtypes must be"),
                       (dict(good, labels=good["labels"].astype(np.int32)), "dtypes must be"),
                       (dict(good, samples=good["samples"].reshape(2, -1)), "one-dimensional"),
                       ({k: v for k, v in good.items() if k != "lengths"}, "array 'lengths' is missing"),
                       ({k: v[:0] if k != "samples" else v for k, v in good.items()}, "no clips")):
        with pytest.raises(ValueError, match=words):
            Fn.check_audio_arrays(bad)
    # an empty clip overlaps nothing, wherever it starts
    Fn.check_audio_arrays(changed("starts", 1, 100))


def test_a_store_that_does_not_fit_is_refused_by_name():
    with pytest.raises(RuntimeError, match=r"AudioStore: the audio store needs 10\.0 MiB.*SPARCH_AUDIO=resident"):
        Fn._require_room(10 * 2**20, 4 * 2**20, "AudioStore", "audio", "SPARCH_AUDIO")
    Fn._require_room(4 * 2**20, 4 * 2**20, "AudioStore", "audio", "SPARCH_AUDIO")
    with pytest.raises(RuntimeError, match="the event store needs.*SPARCH_EVENTS=resident"):   # the event wording stays
        Fn._require_room(10 * 2**20, 4 * 2**20, "EventStore")


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_pack_round_trip_is_byte_identical(tmp_path, dtype):
    a = good_arrays(dtype)
    path = str(tmp_path / "sc_training.audio.npz")
    Fn.save_audio_pack(path, a)
    b = Fn.load_audio_pack(path)
    for k in Fn.AUDIO_PACK_KEYS:
        assert b[k].dtype == a[k].dtype and b[k].shape == a[k].shape and b[k].tobytes() == a[k].tobytes(), k
    with zipfile.ZipFile(path) as z:                             # uncompressed: stored, not deflated
        assert all(i.compress_type == zipfile.ZIP_STORED for i in z.infolist())
        assert sorted(i.filename for i in z.infolist()) == sorted(k + ".npy" for k in Fn.AUDIO_PACK_KEYS)
    Fn.save_audio_pack(str(tmp_path / "again.npz"), b)
    assert open(path, "rb").read() == open(tmp_path / "again.npz", "rb").read()
    # a malformed store is not written, a file that is not a pack is not read
    bad = dict(a, starts=a["starts"] - 10)
    with pytest.raises(ValueError, match="negative start"):
        Fn.save_audio_pack(str(tmp_path / "never.npz"), bad)
    assert not os.path.exists(tmp_path / "never.npz")
    with open(tmp_path / "other.npz", "wb") as f:
        np.savez(f, samples=a["samples"], starts=a["starts"])
    with pytest.raises(ValueError, match="not an audio pack"):
        Fn.load_audio_pack(str(tmp_path / "other.npz"))


def _check_pack(path, files, labels):
    """The pack holds the clips `files` in order: samples as read_clip returns them, labels as listed."""
    a = Fn.load_audio_pack(path)
    assert len(a["labels"]) == len(files) and a["labels"].tolist() == list(labels)
    assert a["starts"][0] == 0 and np.array_equal(a["starts"][1:], np.cumsum(a["lengths"][:-1]))   # no gaps
    assert int(a["starts"][-1] + a["lengths"][-1]) == len(a["samples"])
    for i, f in enumerate(files):
        x, _ = read_clip(f)
        got = a["samples"][a["starts"][i]:a["starts"][i] + a["lengths"][i]]
        if a["samples"].dtype == np.int16:
            assert x.dtype == np.int16 and np.array_equal(got, x), f
        else:
            want = x if x.dtype == np.float32 else x.astype(np.float32) / np.float32(2 ** 15)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), f
    return a


def test_pack_audio_tool_on_an_sc_tree(tmp_path, capsys):
    import pack_audio

    root = str(tmp_path / "sc")
    make_sc_tree(root, n_train=3, n_valid=2, n_test=1, lengths=LENGTHS)
    pack_audio.main([root, "sc"])
    said = capsys.readouterr().out
    for split in ("training", "validation", "testing"):
        ds = nd.SpeechCommands(root, split, False, 0.0001, 0.9, 0.1, device="cpu")
        path = f"{root}/sc_{split}.audio.npz"
        assert path == nd._audio_pack_path(root, "sc", split) and path in said
        a = _check_pack(path, ds.file_list, ds.targets)
        assert a["samples"].dtype == np.int16
    assert len(ds) == 3 and len(set(a["lengths"].tolist())) > 1       # clips of different lengths


def test_pack_audio_tool_on_an_hd_tree(tmp_path):
    import pack_audio

    root = str(tmp_path / "hd")
    make_hd_tree(root, n_train=7, n_test=3, lengths=LENGTHS)
    pack_audio.main([root, "hd"])
    assert sorted(f for f in os.listdir(root) if f.endswith(".npz")) == ["hd_test.audio.npz", "hd_train.audio.npz"]
    for split in ("train", "test"):
        ds = nd.HeidelbergDigits(root, split, False, 0.0001, 0.9, 0.1, device="cpu")
        _check_pack(f"{root}/hd_{split}.audio.npz", ds.file_list, ds.targets)


@pytest.mark.parametrize("odd", ["24bit", "stereo"])
def test_one_clip_that_is_not_16_bit_mono_makes_the_store_fp32(tmp_path, odd):
    root = str(tmp_path / "hd")
    files = make_hd_tree(root, n_train=5, n_test=2, lengths=LENGTHS)
    name = files["train"][2][0]
    g = np.random.default_rng(5)
    if odd == "24bit":
        write_pcm_wav(os.path.join(root, "audio", name), g.integers(-2**23, 2**23, 3000), 3)
    else:
        write_pcm_wav(os.path.join(root, "audio", name), g.integers(-2**15, 2**15, (3000, 2)), 2)
    ds = nd.HeidelbergDigits(root, "train", False, 0.0001, 0.9, 0.1, device="cpu")
    a = Fn.audio_arrays_from_files(ds.file_list, ds.targets, device=None)
    assert a["samples"].dtype == np.float32 and a["lengths"][2] == 3000
    for i, f in enumerate(ds.file_list):
        x, _ = read_clip(f)
        assert (x.dtype == np.float32) == (i == 2)
        want = x if i == 2 else x.astype(np.float32) / np.float32(2 ** 15)
        got = a["samples"][a["starts"][i]:a["starts"][i] + a["lengths"][i]]
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert float(np.abs(a["samples"]).max()) <= 1.0
    ds = nd.HeidelbergDigits(root, "test", False, 0.0001, 0.9, 0.1, device="cpu")     # the other split stays int16
    assert Fn.audio_arrays_from_files(ds.file_list, ds.targets, device=None)["samples"].dtype == np.int16


def test_flac_clips_need_a_device_and_the_refusal_names_the_file(tmp_path):
    root = str(tmp_path / "hd")
    fw.make_hd_flac_tree(root, n_train=4, n_test=2, lengths=(4000, 3000), flac_every=2)
    ds = nd.HeidelbergDigits(root, "train", False, 0.0001, 0.9, 0.1, device="cpu")
    first_flac = next(f for f in ds.file_list if f.endswith(".flac"))
    with pytest.raises(RuntimeError, match=re.escape(first_flac) + ".*no HIP device is visible"):
        Fn.audio_arrays_from_files(ds.file_list, ds.targets, device=None)


def test_sample_rate_warning_once_per_dataset(tmp_path, caplog):
    root = str(tmp_path / "hd")
    make_hd_tree(root, n_train=4, n_test=2, lengths=(4000,), rate=8000)
    ds = nd.HeidelbergDigits(root, "train", False, 0.0001, 0.9, 0.1, device="cpu")
    with caplog.at_level("WARNING"):
        Fn.audio_arrays_from_files(ds.file_list, ds.targets, device=None)
    assert caplog.text.count("sample rate 8000 Hz") == 1


# ----------------------------------------------------------------------------------------- the option
def test_option_parsing(tmp_path, monkeypatch):
    root = str(tmp_path / "sc")
    make_sc_tree(root, lengths=(4000,))
    monkeypatch.setenv("SPARCH_AUDIO", "bogus")
    with pytest.raises(ValueError, match="SPARCH_AUDIO / resident: unknown value 'bogus'"):
        nd.load_hd_or_sc("sc", root, "train", 4, device="cpu")
    with pytest.raises(ValueError, match="unknown value 'yes'"):
        nd.load_hd_or_sc("sc", root, "train", 4, device="cpu", resident="yes")
    for value in (None, ""):
        if value is None:
            monkeypatch.delenv("SPARCH_AUDIO")
        else:
            monkeypatch.setenv("SPARCH_AUDIO", value)
        loader = nd.load_hd_or_sc("sc", root, "train", 4, device="cpu")
        assert type(loader) is nd._EpochCheckedLoader and isinstance(loader.dataset, nd.SpeechCommands)
        assert loader.collate_fn == loader.dataset.generateBatch
    # read when the loader is built, and an explicit argument wins over the environment
    monkeypatch.setenv("SPARCH_AUDIO", "resident")
    assert type(nd.load_hd_or_sc("sc", root, "train", 4, device="cpu", resident="")) is nd._EpochCheckedLoader
    # the names are re-exported, and the event loader keeps its own
    import sparch.dataloaders.nonspiking_datasets as shim
    assert shim.ResidentAudioLoader is nd.ResidentAudioLoader and shim.load_hd_or_sc is nd.load_hd_or_sc
    assert sd._index_loader is _index._index_loader is nd._index_loader
    assert sd._SampleIndices is _index._SampleIndices


# ----------------------------------------------------------------------------------------- C ABI
def test_entry_points_are_declared_and_bound_and_the_abi_is_still_5():
    text = open(os.path.join(ROOT, "include", "sparch_hip.h")).read()
    for name in ("sparch_audio_gather_fbank", "sparch_audio_gather_augment"):
        assert re.search(rf"\bint {name}\s*\(", text), name
        assert name in _capi.PROTOTYPES and hasattr(_capi.lib, name)
    assert _capi.lib.sparch_abi_version() == 5


def test_gather_fbank_argument_checks_return_einval_without_a_device():
    f = _capi.lib.sparch_audio_gather_fbank
    p = 64                                                      # any non-null address: nothing is launched
    good = dict(samples=p, dtype=1, starts=p, lengths=p, labels=p, n_store=10, idx=p, batch=4, n_frames=98,
                n_mels=40, out=p, y=p)

    def call(**change):
        a = dict(good, **change)
        return f(a["samples"], a["dtype"], a["starts"], a["lengths"], a["labels"], a["n_store"], a["idx"],
                 a["batch"], a["n_frames"], a["n_mels"], a["out"], a["y"], None)

    for bad in (dict(samples=None), dict(starts=None), dict(lengths=None), dict(labels=None), dict(idx=None),
                dict(out=None), dict(batch=0), dict(batch=-3), dict(n_mels=0), dict(n_mels=257), dict(dtype=2),
                dict(dtype=-1), dict(n_frames=0), dict(n_store=0),
                dict(batch=2**30, n_frames=98)):                # grid above INT_MAX
        assert call(**bad) == -1, bad


def test_gather_augment_argument_checks_return_einval_without_a_device():
    f = _capi.lib.sparch_audio_gather_augment
    p = 64
    good = dict(samples=p, dtype=0, starts=p, lengths=p, labels=p, n_store=10, idx=p, batch=4, ld=16000, params=p,
                rate=16000, out=p, out_lengths=p, y=p)

    def call(**change):
        a = dict(good, **change)
        return f(a["samples"], a["dtype"], a["starts"], a["lengths"], a["labels"], a["n_store"], a["idx"],
                 a["batch"], a["ld"], a["params"], 0.0001, 0.9, 7, a["rate"], a["out"], a["out_lengths"], a["y"],
                 None)

    for bad in (dict(samples=None), dict(starts=None), dict(lengths=None), dict(labels=None), dict(idx=None),
                dict(params=None), dict(out=None), dict(out_lengths=None), dict(batch=0), dict(ld=0), dict(dtype=2),
                dict(rate=7999), dict(rate=48001), dict(n_store=-1)):
        assert call(**bad) == -1, bad


# ----------------------------------------------------------------------------------------- index lists and draws
class _HostStore:
    """Stands in for an AudioStore on a machine without a GPU: records what each batch is asked for."""
    device = "cpu"

    def __init__(self, n):
        self.n, self.asked = n, []

    def __len__(self):
        return self.n

    def batch(self, idx, idx_host, augment=None, sample_rate=16000):
        assert torch.equal(idx, idx_host) and idx.dtype == torch.int64 and sample_rate == 16000
        self.asked.append((idx_host.tolist(), None if augment is None else (augment[0].copy(), augment[1])))
        return self.asked[-1]


def _states():
    return random.getstate(), torch.get_rng_state().clone(), np.random.get_state()


def _same_states(a, b):
    return a[0] == b[0] and torch.equal(a[1], b[1]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))


def _epochs(which, n, batch_size, shuffle, rank, world, augment, epochs=2):
    """Per epoch: ([(indices, draws)] per batch, generator states after the epoch); `today` draws inside the collate
    function of a DataLoader built by _index_loader, as the file loader does."""
    random.seed(3)
    torch.manual_seed(4)
    np.random.seed(5)

    def collate(batch):
        draws = None if augment is None else draw_augmentation(len(batch), *augment)
        return [int(i) for i in batch], draws

    if which == "today":
        loader = _index._index_loader(_index._SampleIndices(n), batch_size, shuffle, rank, world, 9, collate_fn=collate)
    else:
        loader = nd.ResidentAudioLoader(_HostStore(n), batch_size, shuffle, rank, world, 9, augment=augment)
    out = []
    for e in range(epochs):
        if world > 1:
            loader.sampler.set_epoch(e)
        out.append((list(loader), _states()))
    assert len(loader) == len(out[0][0])
    return out


@pytest.mark.parametrize("augment", [None, (0.0001, 0.9, 0.5)])
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("rank,world", [(0, 1), (0, 2), (1, 2)])
def test_index_lists_and_draws_equal_drawing_inside_the_collate_function(rank, world, shuffle, augment):
    today = _epochs("today", 23, 4, shuffle, rank, world, augment)
    resident = _epochs("resident", 23, 4, shuffle, rank, world, augment)
    for (batches_t, states_t), (batches_r, states_r) in zip(today, resident):
        assert len(batches_t) == len(batches_r) == (6 if world == 1 else 3)
        for (idx_t, draw_t), (idx_r, draw_r) in zip(batches_t, batches_r):
            assert idx_t == idx_r
            if augment is None:
                assert draw_t is None and draw_r is None
            else:
                assert draw_t[1] == draw_r[1] and draw_t[0].tobytes() == draw_r[0].tobytes()
        assert len(batches_r[-1][0]) == (3 if world == 1 else 4)      # 23 = 5 x 4 + 3; 12 per rank = 3 x 4
        assert _same_states(states_t, states_r), "a generator differs after the epoch"
    if shuffle:
        assert [b[0] for b in today[0][0]] != [b[0] for b in today[1][0]]     # a fresh permutation per epoch
    if augment is not None:
        assert not _same_states(today[0][1], today[1][1])


def test_the_file_loader_is_built_with_the_index_loaders_arguments(tmp_path):
    """Same sampler class, batch size and drop_last as the resident loader's DataLoader, for world 1 and 2."""
    root = str(tmp_path / "hd")
    make_hd_tree(root, n_train=7, n_test=3, lengths=(4000,))
    for shuffle in (False, True):
        for rank, world in ((0, 1), (1, 2)):
            real = nd.load_hd_or_sc("hd", root, "train", 4, shuffle=shuffle, device="cpu", rank=rank, world=world,
                                    seed=9, resident="")
            res = nd.ResidentAudioLoader(_HostStore(7), 4, shuffle, rank, world, 9)
            assert type(real.sampler) is type(res.sampler) and real.batch_size == res.index_loader.batch_size
            assert real.drop_last == res.index_loader.drop_last and len(real) == len(res)
            if world > 1:
                assert (real.sampler.seed, real.sampler.shuffle, real.sampler.rank) == \
                    (res.sampler.seed, res.sampler.shuffle, res.sampler.rank)

