"""GPU: the resident HD / SC audio store (SPARCH_AUDIO=resident).  `sparch_audio_gather_fbank` against `fbank_padded`
and `sparch_audio_gather_augment` against `augment_padded` on the gathered rows; the resident loader against the file
loader batch by batch; a store from a pack against a store from files; a network on a resident batch; run_exp.py.
Every comparison is exact (bit patterns): the feature adds no arithmetic."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import flac_writer as fw
from tests.audio_trees import make_hd_tree, make_sc_tree
from tests.kit import DEV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FBANK_LENGTHS = [0, 399, 400, 401, 559, 560, 16000, 16001]
AUGM_LENGTHS = [0, 1, 2, 399, 400, 5000, 16000, 16001]
TREE_LENGTHS = (16000, 9000, 401, 12345, 7000, 20000, 300)     # HD trees: one clip in seven is too short for a frame
SC_LENGTHS = (16000, 9000, 401, 12345, 7000, 300)              # SC trees (a period that spreads over the splits)
TRAIN_BATCH = {"sc": 5, "hd": 4}                               # 12 = 5 + 5 + 2 clips, 11 = 4 + 4 + 3
EVAL_BATCH = {("sc", "valid"): 4, ("sc", "test"): 2, ("hd", "valid"): 2, ("hd", "test"): 2}   # 6, 3, 5, 5 clips


def _bits(t):
    return t.contiguous().view(torch.int32)


def _store(dtype, lengths, seed=0):
    """(AudioStore, clips): clips of `lengths` samples at odd and even start offsets, a few samples of another value
    between them (fp32: NaN, int16: full scale) which no clip owns."""
    from sparch_amd import functional as Fn

    g = np.random.default_rng(seed)
    gaps = [1, 3, 2, 5, 1, 7, 4, 9]
    starts, at = [], 0
    for i, n in enumerate(lengths):
        at += gaps[i % len(gaps)]
        starts.append(at)
        at += n
    assert any(s % 2 for s in starts) and any(s % 2 == 0 for s in starts)
    if dtype == "int16":
        samples = np.full(at + 11, 32767, np.int16)
        clips = [np.round(0.3 * 32767 * np.sin(np.arange(n) * (0.02 + 0.01 * i)) + g.integers(-3000, 3000, n))
                 .astype(np.int16) for i, n in enumerate(lengths)]
    else:   # beyond +-1 on purpose, as in tests/test_augment_gpu.py
        samples = np.full(at + 11, np.nan, np.float32)
        clips = [(g.uniform(-1.3, 1.3, n) * np.sin(np.arange(n) / (40.0 + i))).astype(np.float32)
                 for i, n in enumerate(lengths)]
    for s, c in zip(starts, clips):
        samples[s:s + len(c)] = c
    arrays = {"samples": samples, "starts": np.array(starts, np.int64), "lengths": np.array(lengths, np.int32),
              "labels": np.arange(len(lengths), dtype=np.int64) * 3 + 1}
    store = Fn.AudioStore(arrays, device=DEV)
    assert store.int16 == (dtype == "int16") and len(store) == len(lengths) and store.source == "arrays"
    return store, clips


def _gathered(store, clips, idx):
    """The padded batch buffer the file loader's collate would upload for the clips `idx` (an index outside the
    store: an empty clip), and their lengths."""
    rows = [clips[i] if 0 <= i < len(clips) else clips[0][:0] for i in idx]
    lens = [len(r) for r in rows]
    host = np.zeros((len(rows), max(max(lens), 1)), np.int16 if store.int16 else np.float32)
    for row, r in zip(host, rows):
        row[:len(r)] = r
    return torch.from_numpy(host).to(DEV), lens


def _check_fbank(store, clips, idx, extra_frames=0):
    from sparch_amd import functional as Fn

    wave, lens = _gathered(store, clips, idx)
    ref, frames = Fn.fbank_padded(wave, lens)
    t_max = ref.shape[1]
    got, y = store.gather_fbank(torch.tensor(idx, dtype=torch.int64, device=DEV), t_max + extra_frames)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (len(idx), t_max + extra_frames, 40)
    assert torch.equal(_bits(got[:, :t_max]), _bits(ref)), [int(b) for b in range(len(idx))
                                                             if not torch.equal(_bits(got[b, :t_max]), _bits(ref[b]))]
    assert int(_bits(got[:, t_max:]).abs().max() if extra_frames else 0) == 0       # exact zeros (+0.0)
    for b, f in enumerate(frames.tolist()):
        assert int(_bits(got[b, f:]).abs().max() if f < got.shape[1] else 0) == 0
        assert f == 0 or bool(torch.isfinite(got[b, :f]).all())
    want_y = [3 * i + 1 if 0 <= i < len(clips) else -1 for i in idx]
    assert y.cpu().tolist() == want_y
    return got, frames


@pytest.mark.parametrize("dtype", ["int16", "fp32"])
def test_gather_fbank_equals_fbank_padded_on_the_gathered_rows(dtype):
    store, clips = _store(dtype, FBANK_LENGTHS)
    n = len(clips)
    every = list(range(n))
    got, frames = _check_fbank(store, clips, every)
    assert frames.tolist() == [0, 0, 1, 1, 1, 2, 98, 98] and float(got.abs().sum()) > 0
    _check_fbank(store, clips, every, extra_frames=9)                    # n_frames_out larger than every clip needs
    _check_fbank(store, clips, [6])                                      # batch of 1
    _check_fbank(store, clips, [2], extra_frames=1)                      # one frame, one frame of padding
    _check_fbank(store, clips, [5, 7, 5, 5, 1, 7, 0, 5])                 # repeated indices
    _check_fbank(store, clips, [7, n, 3, -1, 6, 10 ** 12, -(10 ** 12)], extra_frames=3)   # outside the store
    got, _ = _check_fbank(store, clips, [n + 5, 6])
    assert float(got[0].abs().sum()) == 0.0                              # zero row for the index outside
    # fewer frames than a clip has: the clip is cut, the frames that are there are the same
    full, _ = store.gather_fbank(torch.tensor([6, 5], dtype=torch.int64, device=DEV), 98)
    cut, _ = store.gather_fbank(torch.tensor([6, 5], dtype=torch.int64, device=DEV), 10)
    assert torch.equal(_bits(cut), _bits(full[:, :10]))


def test_int16_and_fp32_stores_give_the_same_bits():
    """What lets the store take the int16 / fp32 decision once per split."""
    from sparch_amd import functional as Fn

    store, clips = _store("int16", FBANK_LENGTHS)
    a = {k: getattr(store, k).cpu().numpy() for k in ("samples", "starts", "lengths", "labels")}
    a["samples"] = a["samples"].astype(np.float32) / np.float32(2 ** 15)
    as_float = Fn.AudioStore(a, device=DEV)
    idx = torch.arange(len(clips), dtype=torch.int64, device=DEV)
    assert torch.equal(_bits(store.gather_fbank(idx, 98)[0]), _bits(as_float.gather_fbank(idx, 98)[0]))


def _augm_table(n, seed):
    """draw_augmentation's table for n clips with every stage applied to some clips and skipped for others."""
    from sparch_amd.dataloaders.augment import draw_augmentation

    for s in range(seed, seed + 1000):
        random.seed(s)
        torch.manual_seed(s)
        np.random.seed(s)
        params, noise_seed = draw_augmentation(n, 0.0001, 0.9, 0.5)
        if all(0 < params[:, c].sum() < n for c in range(4)):
            return params, noise_seed
    raise AssertionError("no seed")


@pytest.mark.parametrize("dtype", ["int16", "fp32"])
def test_gather_augment_equals_augment_padded_on_the_gathered_rows(dtype):
    from sparch_amd import functional as Fn
    from sparch_amd._capi import lib, ptr

    store, clips = _store(dtype, AUGM_LENGTHS, seed=1)
    n = len(clips)
    for idx in (list(range(n)), [6, 7, 6, 5, n + 2, 0, -1, 6, 4, 3], [7]):
        params, noise_seed = _augm_table(max(len(idx), 4), 10)
        params = params[:len(idx)]
        wave, lens = _gathered(store, clips, idx)
        ld = wave.shape[1]
        ref = Fn.augment_padded(wave, lens, params, noise_seed, 0.0001, 0.9)
        rows, lens_dev, y = store.gather_augment(torch.tensor(idx, dtype=torch.int64, device=DEV), ld, params,
                                                 noise_seed, 0.0001, 0.9)
        torch.cuda.synchronize()
        assert lens_dev.dtype == torch.int32 and lens_dev.cpu().tolist() == lens
        assert y.cpu().tolist() == [3 * i + 1 if 0 <= i < n else -1 for i in idx]
        for b, m in enumerate(lens):
            assert torch.equal(_bits(rows[b, :m]), _bits(ref[b, :m])), (idx[b], m, params[b].tolist())
            assert m == 0 or bool(torch.isfinite(rows[b, :m]).all())
        # a row is not written behind its clip (raw call into a NaN-filled buffer)
        out = torch.full((len(idx), ld), float("nan"), device=DEV)
        idx_d = torch.tensor(idx, dtype=torch.int64, device=DEV)
        prm = torch.from_numpy(params).to(DEV)
        st = lib.sparch_audio_gather_augment(ptr(store.samples), store.dtype, ptr(store.starts), ptr(store.lengths),
                                             ptr(store.labels), len(store), ptr(idx_d), len(idx), ld, ptr(prm), 0.0001,
                                             0.9, noise_seed, 16000, ptr(out), ptr(lens_dev), ptr(y),
                                             torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert st == 0
        for b, m in enumerate(lens):
            assert torch.equal(_bits(out[b, :m]), _bits(ref[b, :m])) and bool(torch.isnan(out[b, m:]).all())
    # the augmented batch of the store: those rows through the padded fbank
    idx = [6, 5, 3, 7]
    params, noise_seed = _augm_table(4, 50)
    wave, lens = _gathered(store, clips, idx)
    ref, frames = Fn.fbank_padded(Fn.augment_padded(wave, lens, params, noise_seed, 0.0001, 0.9), lens)
    host_idx = torch.tensor(idx, dtype=torch.int64)
    xs, xlens, ys = store.batch(host_idx.to(DEV), host_idx, augment=(params, noise_seed, 0.0001, 0.9))
    assert torch.equal(_bits(xs), _bits(ref)) and torch.equal(xlens, frames) and xlens.dtype == frames.dtype
    assert not xlens.is_cuda and ys.is_cuda and ys.cpu().tolist() == [19, 16, 10, 22]
    plain = store.batch(host_idx.to(DEV), host_idx)[0]
    assert plain.shape == xs.shape and not torch.equal(_bits(plain), _bits(xs))


def test_store_argument_checks():
    from sparch_amd import functional as Fn

    store, clips = _store("int16", [400, 100, 200])
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    for bad in (idx.int(), idx.cpu(), idx[:0], torch.zeros(2, 2, dtype=torch.int64, device=DEV)):
        with pytest.raises((ValueError, RuntimeError)):
            store.gather_fbank(bad, 3)
    with pytest.raises(ValueError):
        store.gather_fbank(idx, 0)                                          # refused by the library
    with pytest.raises(ValueError, match="params must be"):
        store.gather_augment(idx, 400, np.zeros((3, 9), np.float32), 0, 0.1, 0.9)
    for field, value, words in ((0, 2.0, "flags"), (4, 1.5, "noise uniform"), (5, float("inf"), "gain ratio"),
                                (7, 101.0, "must lie in")):     # what augment_padded refuses, refused here too
        table = np.zeros((2, 9), np.float32)
        table[1, field] = value
        with pytest.raises(ValueError, match=words):
            store.gather_augment(idx, 400, table, 0, 0.1, 0.9)
    with pytest.raises(ValueError, match="sample rate"):
        store.gather_augment(idx, 400, np.zeros((2, 9), np.float32), 0, 0.1, 0.9, sample_rate=96000)
    host = torch.tensor([1, 2], dtype=torch.int64)
    with pytest.raises(ValueError, match="no clip is long enough for one frame"):   # fbank_padded's refusal
        store.batch(host.to(DEV), host)
    with pytest.raises(ValueError, match="negative start"):
        Fn.AudioStore({"samples": np.zeros(4, np.int16), "starts": np.array([-1], np.int64),
                       "lengths": np.array([2], np.int32), "labels": np.array([0], np.int64)}, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.AudioStore({"samples": np.zeros(4, np.int16), "starts": np.array([0], np.int64),
                       "lengths": np.array([2], np.int32), "labels": np.array([0], np.int64)}, device="cpu")


# ----------------------------------------------------------------------------------------- loaders
def _tree(kind, root):
    """A small tree of `kind`; returns the dataset name."""
    if kind == "sc":
        make_sc_tree(root, n_train=4, n_valid=2, n_test=1, lengths=SC_LENGTHS)         # 12 training clips
        return "sc"
    if kind == "hd_wav":
        make_hd_tree(root, n_train=11, n_test=5, lengths=TREE_LENGTHS)
    else:
        fw.make_hd_flac_tree(root, n_train=11, n_test=5, lengths=TREE_LENGTHS, flac_every=2 if kind == "hd_mix" else 1,
                             blocks=1024)
    return "hd"


def _seed_all(s):
    random.seed(s)
    torch.manual_seed(s + 1)
    np.random.seed(s + 2)


def _states():
    return random.getstate(), torch.get_rng_state().clone(), np.random.get_state()


def _same_states(a, b):
    return a[0] == b[0] and torch.equal(a[1], b[1]) and all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))


def _run(loader, epochs=2, seed=21):
    _seed_all(seed)
    out = []
    for e in range(epochs):
        if hasattr(loader.sampler, "set_epoch"):
            loader.sampler.set_epoch(e)
        out.append([(xs.cpu(), xlens, ys.cpu(), xs.is_cuda, ys.is_cuda) for xs, xlens, ys in loader])
    return out, _states()


def _compare(file_epochs, res_epochs, batch_size):
    assert len(file_epochs) == len(res_epochs)
    for today, res in zip(file_epochs, res_epochs):
        assert len(today) == len(res) > 1
        for (x0, l0, y0, _, _), (x1, l1, y1, x_dev, y_dev) in zip(today, res):
            assert x_dev and y_dev and not l1.is_cuda
            assert x0.shape == x1.shape and torch.equal(_bits(x0), _bits(x1))
            assert torch.equal(l0, l1) and l0.dtype == l1.dtype == torch.int64
            assert torch.equal(y0, y1) and y0.dtype == y1.dtype
        assert 0 < len(res[-1][2]) < batch_size                                    # the short last batch


@pytest.mark.parametrize("augm", [False, True])
@pytest.mark.parametrize("kind", ["sc", "hd_wav", "hd_flac", "hd_mix"])
def test_resident_loader_equals_the_file_loader(tmp_path, monkeypatch, caplog, kind, augm):
    from sparch_amd.dataloaders.nonspiking_datasets import ResidentAudioLoader, load_hd_or_sc

    root = str(tmp_path / kind)
    name = _tree(kind, root)
    if augm:
        monkeypatch.setenv("SPARCH_AUGMENT", "restated")
    kw = dict(shuffle=True, use_augm=augm, p_noise=0.5, device=DEV)
    batch = TRAIN_BATCH[name]
    runs = {}
    for resident in ("", "resident"):
        with caplog.at_level("INFO"):
            loader = load_hd_or_sc(name, root, "train", batch, resident=resident, **kw)
        assert isinstance(loader, ResidentAudioLoader) == (resident == "resident") and len(loader) == 3
        runs[resident] = _run(loader)
    assert re.search(r"Clips of the \w+ \w+ set are resident on cuda(:0)?: 1[12] clips, \d+\.\d MiB, int16 samples, "
                     r"from the files", caplog.text)
    assert ("augmented per batch on the device" in caplog.text) == augm
    _compare(runs[""][0], runs["resident"][0], batch)
    assert _same_states(runs[""][1], runs["resident"][1]), "a generator differs after the epochs"
    first, second = ([b[2].tolist() for b in e] for e in runs["resident"][0])
    assert first != second                                                         # shuffled afresh per epoch
    if augm:   # the augmentation is there: not the plain batches
        plain = _run(load_hd_or_sc(name, root, "train", batch, resident="resident", shuffle=True, device=DEV))[0]
        assert not all(torch.equal(_bits(a[0]), _bits(b[0])) for a, b in zip(plain[0], runs["resident"][0][0]))
    # the other splits are not augmented, and equal too
    for split in ("valid", "test"):
        small = EVAL_BATCH[name, split]
        a = _run(load_hd_or_sc(name, root, split, small, resident="", **dict(kw, shuffle=False)), epochs=1)
        b = _run(load_hd_or_sc(name, root, split, small, resident="resident", **dict(kw, shuffle=False)), epochs=1)
        _compare(a[0], b[0], small)
        assert _same_states(a[1], b[1])


def test_environment_variable_selects_the_resident_loader(tmp_path, monkeypatch):
    from sparch_amd.dataloaders.nonspiking_datasets import ResidentAudioLoader, load_hd_or_sc

    root = str(tmp_path / "hd")
    make_hd_tree(root, n_train=5, n_test=2, lengths=TREE_LENGTHS)
    monkeypatch.setenv("SPARCH_AUDIO", "resident")
    loader = load_hd_or_sc("hd", root, "train", 4, device=DEV)
    assert isinstance(loader, ResidentAudioLoader) and not hasattr(loader, "values") and hasattr(loader, "store")
    assert sum(len(y) for _, _, y in loader) == 5


def test_an_fp32_store_serves_the_file_loaders_batches(tmp_path):
    """One 24-bit FLAC clip: the store is fp32 for the whole split, the file loader decides per batch."""
    from sparch_amd.dataloaders.nonspiking_datasets import load_hd_or_sc

    root = str(tmp_path / "hd")
    files = fw.make_hd_flac_tree(root, n_train=9, n_test=2, lengths=TREE_LENGTHS, flac_every=2, blocks=1024)
    g = np.random.default_rng(3)
    fw.write_flac(os.path.join(root, "audio", files["train"][2][0]), g.integers(-2 ** 22, 2 ** 22, 6000), 24,
                  blocks=1024)
    runs = {}
    for resident in ("", "resident"):
        loader = load_hd_or_sc("hd", root, "train", 4, shuffle=False, device=DEV, resident=resident)
        runs[resident] = _run(loader, epochs=1)
    assert not loader.store.int16
    _compare(runs[""][0], runs["resident"][0], 4)


def test_a_corrupt_flac_file_raises_at_load_naming_the_file(tmp_path):
    from sparch_amd.dataloaders.audio import FlacError
    from sparch_amd.dataloaders.nonspiking_datasets import load_hd_or_sc

    root = str(tmp_path / "hd")
    expect = fw.make_hd_flac_tree(root, n_train=6, n_test=1, lengths=TREE_LENGTHS)
    victim = os.path.join(root, "audio", expect["train"][4][0])
    data = bytearray(open(victim, "rb").read())
    data[len(data) // 2] ^= 0x01
    open(victim, "wb").write(bytes(data))
    with pytest.raises(FlacError) as e:
        load_hd_or_sc("hd", root, "train", 2, shuffle=False, device=DEV, resident="resident")
    assert victim in str(e.value)
    load_hd_or_sc("hd", root, "test", 2, shuffle=False, device=DEV, resident="resident")     # the other split loads
    fw.make_hd_flac_tree(str(tmp_path / "bad"), n_train=4, n_test=1, md5=b"\x01" * 16)
    with pytest.raises(FlacError, match="MD5") as e:
        load_hd_or_sc("hd", str(tmp_path / "bad"), "train", 4, shuffle=False, device=DEV, resident="resident")
    assert "lang-" in str(e.value) and ".flac" in str(e.value)


@pytest.mark.parametrize("kind", ["sc", "hd_mix"])
def test_store_from_a_pack_equals_the_store_from_files(tmp_path, caplog, kind):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pack_audio
    from sparch_amd.dataloaders.nonspiking_datasets import load_hd_or_sc

    root = str(tmp_path / kind)
    name = _tree(kind, root)
    batch = TRAIN_BATCH[name]
    from_files = load_hd_or_sc(name, root, "train", batch, shuffle=True, device=DEV, resident="resident")
    assert from_files.store.source == "files"
    pack_audio.main([root, name])                      # the FLAC clips of hd_mix are decoded on the device
    with caplog.at_level("INFO"):
        from_pack = load_hd_or_sc(name, root, "train", batch, shuffle=True, device=DEV, resident="resident")
    assert from_pack.store.source == "pack" and "from the pack " + root in caplog.text
    for k in ("samples", "starts", "lengths", "labels"):
        a, b = getattr(from_files.store, k), getattr(from_pack.store, k)
        assert a.dtype == b.dtype and torch.equal(a, b), k
    assert torch.equal(from_files.store.lengths_host, from_pack.store.lengths_host)
    a, b = _run(from_files), _run(from_pack)
    _compare(a[0], b[0], batch)
    assert _same_states(a[1], b[1])
    # a pack that no longer matches the file list is refused
    if name == "hd":
        lines = open(os.path.join(root, "train_filenames.txt")).read().splitlines()
        open(os.path.join(root, "train_filenames.txt"), "w").write("\n".join(lines[1:]) + "\n")
    else:
        os.remove(os.path.join(root, "yes", "00_nohash_0.wav"))          # a training clip
    with pytest.raises(ValueError, match="write the pack again"):
        load_hd_or_sc(name, root, "train", 4, device=DEV, resident="resident")


@pytest.mark.parametrize("shuffle", [False, True])
def test_the_two_ranks_shares_equal_the_file_loaders(tmp_path, shuffle):
    from sparch_amd.dataloaders.nonspiking_datasets import load_hd_or_sc

    root = str(tmp_path / "hd")
    make_hd_tree(root, n_train=11, n_test=3, lengths=TREE_LENGTHS)
    labels = []
    for rank in (0, 1):
        kw = dict(shuffle=shuffle, device=DEV, rank=rank, world=2, seed=13)
        a = _run(load_hd_or_sc("hd", root, "train", 4, resident="", **kw))
        b = _run(load_hd_or_sc("hd", root, "train", 4, resident="resident", **kw))
        assert len(a[0][0]) == 2 and [len(x[2]) for x in b[0][0]] == [4, 2]       # 11 clips padded to 12, 6 per rank
        _compare(a[0], b[0], 4)
        assert _same_states(a[1], b[1])
        labels.append([y for batch in b[0][0] for y in batch[2].tolist()])
    assert len(labels[0]) == len(labels[1]) == 6


def test_network_on_a_resident_batch_equals_the_file_loaders_batch(tmp_path):
    import sparch_amd
    from sparch_amd import functional as Fn
    from sparch_amd.dataloaders.nonspiking_datasets import load_hd_or_sc

    root = str(tmp_path / "sc")
    make_sc_tree(root, n_train=3, n_valid=1, n_test=1, lengths=SC_LENGTHS)
    xs = []
    for resident in ("", "resident"):
        loader = load_hd_or_sc("sc", root, "train", 8, shuffle=False, device=DEV, resident=resident)
        x, _, y = next(iter(loader))
        xs.append((x.to(DEV), y.to(DEV)))
    torch.manual_seed(2)
    net = sparch_amd.SNN((8, None, 40), [64, 48, 3], neuron_type="RadLIF", dropout=0.0).to(DEV).train()
    res = []
    for x, y in xs:
        net.zero_grad()
        torch.manual_seed(5)
        out, rates = net(x)
        torch.nn.functional.cross_entropy(out, y).backward()
        Fn.check_status()
        res.append((out.detach().clone(), rates.detach().clone(),
                    {k: v.grad.clone() for k, v in net.named_parameters()}))
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and torch.equal(_bits(res[0][1]), _bits(res[1][1]))
    assert bool(torch.isfinite(res[0][0]).all())
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k


@pytest.mark.parametrize("name,augm", [("sc", "0"), ("hd", "1")])
def test_run_exp_with_resident_audio(tmp_path, name, augm):
    """run_exp.py in a fresh child process: two epochs from the resident store (hd: FLAC files, augmented)."""
    data = str(tmp_path / name)
    if name == "sc":
        make_sc_tree(data, n_train=4, n_valid=2, n_test=2, lengths=SC_LENGTHS)
    else:
        fw.make_hd_flac_tree(data, n_train=10, n_test=6, lengths=TREE_LENGTHS, blocks=1024)
    exp = tmp_path / "exp"
    env = dict(os.environ, SPARCH_AUDIO="resident", SPARCH_AUGMENT="restated")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_exp.py"), "--dataset_name", name, "--data_folder", data,
                        "--nb_epochs", "2", "--model_type", "RadLIF", "--nb_hiddens", "64", "--batch_size", "4",
                        "--use_augm", augm, "--log_tofile", "1", "--new_exp_folder", str(exp)],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    log = (exp / "log" / "exp.log").read_text()
    train = "training" if name == "sc" else "train"
    for line in (f"Clips of the {name} {train} set are resident on", "int16 samples, from the files",
                 "Epoch 1: train loss=", "Epoch 2: train loss=", "Epoch 2: valid acc=", "Test acc="):
        assert line in log, line
    assert ("augmented per batch on the device" in log) == (augm == "1")
    losses = [float(v) for v in re.findall(r"Epoch \d+: train loss=(\S+)", log)]
    assert len(losses) == 2 and all(np.isfinite(losses)) and "nan" not in log.lower()
