"""CPU: the HD / SC file loaders (sparch_amd/dataloaders/nonspiking_datasets.py, audio.py) up to the host samples
(`__getitem__` touches no GPU): WAV decoding against torchaudio's documented normalisation (unpinned: torchaudio is
not installed), the reference's file lists, their order and labels, the loader's refusals and its data-parallel
shares, and the argument checks of sparch_fbank_padded_fwd (no launch)."""
import logging
import os

import numpy as np
import pytest

from sparch_amd import _capi
from sparch_amd.dataloaders import audio
from sparch_amd.dataloaders.nonspiking_datasets import (HeidelbergDigits, SpeechCommands, hd_label,
                                                         load_hd_or_sc)
from tests.audio_trees import hd_name, make_hd_tree, make_sc_tree, write_pcm_wav, write_raw_wav

# ----------------------------------------------------------------------------------------- WAV decoding
_INT_RANGE = {1: (0, 255), 2: (-2 ** 15, 2 ** 15 - 1), 3: (-2 ** 23, 2 ** 23 - 1), 4: (-2 ** 31, 2 ** 31 - 1)}


def _expected(frames, width):
    """The normalisation table on channel 0, in float64, rounded once to float32."""
    x = frames[:, 0].astype(np.float64)
    return ((x - 128) / 128 if width == 1 else x / 2.0 ** (8 * width - 1)).astype(np.float32)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_pcm_wav_normalisation_and_channel_0(tmp_path, width, channels):
    lo, hi = _INT_RANGE[width]
    g = np.random.default_rng(width * 10 + channels)
    frames = g.integers(lo, hi, size=(500, channels), endpoint=True, dtype=np.int64)
    frames[:4, 0] = [lo, hi, (lo + hi + 1) // 2, (lo + hi + 1) // 2 - 1]   # both extremes and the two around zero
    path = tmp_path / "clip.wav"
    write_pcm_wav(path, frames, width, rate=16000)
    x, rate = audio.read_audio(str(path))
    assert rate == 16000 and x.shape == (500,)
    if width == 2 and channels == 1:  # stays int16 up to the device
        assert x.dtype == np.int16 and np.array_equal(x, frames[:, 0])
    else:
        assert x.dtype == np.float32 and np.array_equal(x, _expected(frames, width))
    xf = x / np.float32(2 ** 15) if x.dtype == np.int16 else x
    assert xf[0] == -1.0 and float(xf.max()) <= 1.0   # (2^31 - 1) / 2^31 rounds to 1.0 in fp32


@pytest.mark.parametrize("extensible", [False, True])
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("channels", [1, 2])
def test_float_wav_read_as_is(tmp_path, bits, channels, extensible):
    g = np.random.default_rng(bits + channels)
    frames = g.uniform(-1, 1, size=(300, channels)).astype(np.float32)
    frames[0, 0] = 1.5                       # float data is not clipped or rescaled
    path = tmp_path / "f.wav"
    write_raw_wav(path, frames, tag=3, bits=bits, rate=16000, extensible=extensible)
    x, rate = audio.read_audio(str(path))
    assert rate == 16000 and x.dtype == np.float32 and np.array_equal(x, frames[:, 0])


@pytest.mark.parametrize("bits", [16, 32])
@pytest.mark.parametrize("channels", [1, 2])
def test_extensible_pcm_wav(tmp_path, bits, channels):
    lo, hi = _INT_RANGE[bits // 8]
    frames = np.random.default_rng(bits).integers(lo, hi, size=(200, channels), endpoint=True, dtype=np.int64)
    path = tmp_path / "e.wav"
    write_raw_wav(path, frames, tag=1, bits=bits, rate=16000, extensible=True)
    x, _ = audio.read_audio(str(path))
    if bits == 16 and channels == 1:
        assert x.dtype == np.int16 and np.array_equal(x, frames[:, 0])
    else:
        assert x.dtype == np.float32 and np.array_equal(x, _expected(frames, bits // 8))


def test_wav_recognised_by_header_not_by_name(tmp_path):
    frames = np.arange(-100, 100, dtype=np.int64)
    path = tmp_path / "digit.flac"                      # a WAV file under another name
    write_pcm_wav(path, frames, 2)
    assert audio.is_wav(str(path))
    x, _ = audio.read_audio(str(path))
    assert np.array_equal(x, frames)


def test_non_wav_file_needs_soundfile(tmp_path):
    try:
        import soundfile  # noqa: F401
        pytest.skip("soundfile is installed here: the missing-package path cannot be taken")
    except ImportError:
        pass
    path = tmp_path / "lang-english_speaker-01_trial-0_digit-3.wav"   # not a WAV file, whatever its name says
    path.write_bytes(b"fLaC" + bytes(64))
    assert not audio.is_wav(str(path))
    with pytest.raises(ImportError, match="soundfile") as e:
        audio.read_audio(str(path))
    assert str(path) in str(e.value)


def test_sample_rate_warning_once_per_dataset(tmp_path, caplog):
    root = str(tmp_path / "hd")
    make_hd_tree(root, n_train=3, n_test=1, lengths=(800,), rate=8000)
    ds = HeidelbergDigits(root, "train", False, 0.0001, 0.9, 0.1)
    with caplog.at_level(logging.WARNING):
        for i in range(len(ds)):
            x, _ = ds[i]
            assert len(x) == 800            # not resampled
    warned = [r for r in caplog.records if "8000 Hz" in r.getMessage()]
    assert len(warned) == 1
    caplog.clear()
    make_sc_tree(str(tmp_path / "sc"))       # 16 kHz: no warning
    ds = SpeechCommands(str(tmp_path / "sc"), "training", False, 0.0001, 0.9, 0.1)
    with caplog.at_level(logging.WARNING):
        ds[0]
    assert not [r for r in caplog.records if "Hz" in r.getMessage()]


# ----------------------------------------------------------------------------------------- Speech Commands
def _rel(ds, root):
    return [os.path.relpath(f, root) for f in ds.file_list]


@pytest.mark.parametrize("form", ["relative", "dot-relative", "absolute"])
def test_sc_file_lists_order_and_labels(tmp_path, monkeypatch, form):
    expect = make_sc_tree(str(tmp_path / "speech"), n_train=3, n_valid=2, n_test=2)
    monkeypatch.chdir(tmp_path)
    folder = {"relative": "speech", "dot-relative": "./speech", "absolute": str(tmp_path / "speech")}[form]
    for split in ("training", "validation", "testing"):
        ds = SpeechCommands(folder, split, False, 0.0001, 0.9, 0.1)
        assert ds.labels == ["no", "up", "yes"]
        assert [os.path.normpath(p) for p in _rel(ds, folder)] == [n for n, _ in expect[split]], split
        assert ds.targets == [y for _, y in expect[split]], split
        for f in ds.file_list:
            assert os.path.exists(f)
        assert ds[0][1] == expect[split][0][1]
    train = SpeechCommands(folder, "training", False, 0.0001, 0.9, 0.1)
    # the validation and testing files (one of them listed as "./<word>/...") and the background noise are out
    assert len(train) == 9 and not any("_background_noise_" in f for f in train.file_list)


def test_sc_loader_split_names_and_log(tmp_path, caplog):
    root = str(tmp_path / "sc")
    expect = make_sc_tree(root)
    with caplog.at_level(logging.INFO):
        for split, name in (("train", "training"), ("valid", "validation"), ("test", "testing")):
            loader = load_hd_or_sc("sc", root, split, 2, shuffle=False)
            assert loader.dataset.targets == [y for _, y in expect[name]]
            assert f"Number of examples in sc {name} set: {len(expect[name])}" in caplog.text
    with pytest.raises(ValueError):
        load_hd_or_sc("sc", root, "validation", 2)
    with pytest.raises(ValueError):
        load_hd_or_sc("shd", root, "train", 2)


# ----------------------------------------------------------------------------------------- Heidelberg Digits
def test_hd_label_rule():
    assert hd_label("lang-german_speaker-02_trial-1_digit-7.flac") == 17
    assert hd_label("lang-english_speaker-11_trial-30_digit-0.flac") == 0
    assert hd_label(hd_name("german", 3, 4, 9)) == 19   # .wav copies too
    assert hd_label("audio/" + hd_name("english", 3, 4, 5)) == 5


def test_hd_lists_labels_and_valid_is_test(tmp_path, caplog):
    root = str(tmp_path / "hd")
    expect = make_hd_tree(root, n_train=6, n_test=4)
    ds = HeidelbergDigits(root, "train", False, 0.0001, 0.9, 0.1)
    assert [os.path.basename(f) for f in ds.file_list] == [n for n, _ in expect["train"]]
    assert ds.targets == [y for _, y in expect["train"]]
    assert {y >= 10 for y in ds.targets} == {True, False}      # German and English names
    assert ds[1][1] == expect["train"][1][1]
    with caplog.at_level(logging.INFO):
        loader = load_hd_or_sc("hd", root, "valid", 2, shuffle=False)
    assert "HD uses the same split for validation and testing." in caplog.text
    assert "Number of examples in hd test set: 4" in caplog.text
    assert loader.dataset.targets == [y for _, y in expect["test"]]
    with pytest.raises(ValueError):
        HeidelbergDigits(root, "valid", False, 0.0001, 0.9, 0.1)


# ----------------------------------------------------------------------------------------- loader options
def test_loader_refuses_workers_and_augmentation(tmp_path):
    root = str(tmp_path / "sc")
    make_sc_tree(root)
    with pytest.raises(ValueError, match="workers"):
        load_hd_or_sc("sc", root, "train", 2, workers=2)
    with pytest.raises(NotImplementedError, match="torchaudio_augmentations"):
        load_hd_or_sc("sc", root, "train", 2, use_augm=True)
    make_hd_tree(str(tmp_path / "hd"))
    with pytest.raises(NotImplementedError, match="torchaudio_augmentations"):
        load_hd_or_sc("hd", str(tmp_path / "hd"), "train", 2, use_augm=True)


@pytest.mark.parametrize("shuffle", [True, False])
def test_two_rank_shares_are_disjoint_and_cover_the_split(tmp_path, shuffle):
    root = str(tmp_path / "sc")
    make_sc_tree(root, n_train=4)                       # 12 training files
    shares = []
    for rank in range(2):
        loader = load_hd_or_sc("sc", root, "train", 3, shuffle=shuffle, rank=rank, world=2, seed=5)
        loader.sampler.set_epoch(1)
        shares.append(list(loader.sampler))
    assert len(shares[0]) == len(shares[1]) == 6
    assert not set(shares[0]) & set(shares[1])
    assert sorted(shares[0] + shares[1]) == list(range(12))


# ----------------------------------------------------------------------------------------- C ABI
def test_fbank_padded_argument_checks_without_launching():
    lib = _capi.lib
    f = lib.sparch_fbank_padded_fwd
    ok = dict(n_clips=2, ld=16000, lengths=8, n_frames_out=98, n_mels=40, in_dtype=0, wave=8, out=8)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["n_clips"], a["ld"], a["lengths"], a["n_frames_out"], a["n_mels"], a["in_dtype"], a["wave"],
                 a["out"], None)

    for bad in (dict(n_clips=0), dict(ld=0), dict(n_frames_out=0), dict(n_mels=0), dict(n_mels=257),
                dict(in_dtype=2), dict(in_dtype=-1), dict(lengths=None), dict(wave=None), dict(out=None),
                dict(n_clips=1 << 30, n_frames_out=1 << 20)):
        assert call(**bad) == -1, bad


# ----------------------------------------------------------------------------------------- trainer options
@pytest.mark.parametrize("dataset", ["hd", "sc"])
def test_sync_bn_refused_for_file_audio_on_several_ranks(tmp_path, monkeypatch, dataset):
    """Each rank's batch is as long as its own longest clip, and the --sync_bn exchange needs equal row counts: the
    trainer refuses the combination on every rank before any collective or folder is made."""
    import run_exp
    from sparch_amd import exp
    monkeypatch.setattr(exp.dp, "init_from_env", lambda: (1, 2, 1))
    folder = str(tmp_path / "exp")
    args = run_exp.parse_args(["--dataset_name", dataset, "--data_folder", str(tmp_path), "--sync_bn", "1",
                               "--new_exp_folder", folder])
    with pytest.raises(ValueError, match="--sync_bn"):
        exp.Experiment(args)
    assert not os.path.exists(folder)
