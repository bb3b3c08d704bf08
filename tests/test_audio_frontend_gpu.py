"""GPU: the variable-length mel front-end (`sparch_amd.fbank_padded`, sparch_fbank_padded_fwd) against the
fixed-length kernel clip by clip (bit for bit) and the NumPy restatement (oracle/fbank_numpy.py, the tolerances of
test_hip_parity.py::test_fbank_vs_numpy_restatement_and_known_answers); the SC loader's batches against the
reference's construction (fbank per clip, then pad_sequence); run_exp.py on SC and HD folder trees."""
import os
import wave

import numpy as np
import pytest
import torch

from oracle import fbank_numpy as fo
from tests.audio_trees import make_hd_tree, make_sc_tree
from tests.kit import DEV

pytestmark = pytest.mark.gpu

LENGTHS = [0, 399, 400, 559, 560, 12345, 16000, 23999]
LD = 24000


def _close_to_oracle(out, wave):
    """The existing fbank test's tolerances: 2e-3 in bins within e^12 of the frame's peak, 2e-2 everywhere."""
    ref = fo.fbank(np.asarray(wave, np.float64))
    assert out.shape == ref.shape
    err = np.abs(out - ref)
    strong = ref >= ref.max(axis=1, keepdims=True) - 12.0
    assert err[strong].max() <= 2e-3, err[strong].max()
    assert err.max() <= 2e-2, err.max()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _frames(n):
    return 0 if n < 400 else 1 + (n - 400) // 160


def test_fbank_padded_per_clip_bits_zeros_and_oracle():
    import sparch_amd as sp
    g = torch.Generator().manual_seed(11)
    t = torch.arange(LD) / 16000.0
    clean = 0.1 * (torch.rand(len(LENGTHS), LD, generator=g) * 2 - 1) + 0.3 * torch.sin(
        2 * np.pi * (300.0 + 170.0 * torch.arange(len(LENGTHS))[:, None]) * t[None])
    wave = clean.clone()
    for i, n in enumerate(LENGTHS):
        wave[i, n:] = float("nan")          # past each clip's end: a read there would poison its frames
    feats, frames = sp.fbank_padded(wave.to(DEV), LENGTHS)
    feats = feats.cpu()
    assert frames.dtype == torch.int64 and frames.tolist() == [_frames(n) for n in LENGTHS]
    assert frames.tolist()[:5] == [0, 0, 1, 1, 2]
    assert feats.shape == (len(LENGTHS), _frames(23999), 40) and feats.dtype == torch.float32
    for i, n in enumerate(LENGTHS):
        f = int(frames[i])
        tail = feats[i, f:]
        assert torch.equal(_bits(tail), torch.zeros_like(_bits(tail))), i   # +0.0f exactly
        if f == 0:
            continue
        alone = sp.fbank(clean[i, :n].to(DEV)).cpu()[0]
        assert torch.equal(_bits(feats[i, :f]), _bits(alone)), i
        _close_to_oracle(feats[i, :f].numpy(), clean[i, :n].numpy())

    # int16 PCM: scaled by 2^-15 on load, the same bits as the fp32 path on pcm / 32768
    pcm = (clean * 32767).round().to(torch.int16)
    for i, n in enumerate(LENGTHS):
        pcm[i, n:] = -32768
    f16, fr16 = sp.fbank_padded(pcm.to(DEV), torch.tensor(LENGTHS))
    f32, fr32 = sp.fbank_padded((pcm.float() / 32768).to(DEV), LENGTHS)
    assert torch.equal(fr16, fr32) and torch.equal(_bits(f16.cpu()), _bits(f32.cpu()))

    # a batch whose longest clip has fewer frames than the row allows: T_max follows the clips, not ld
    short, fr = sp.fbank_padded(wave[:4].to(DEV), LENGTHS[:4])
    assert short.shape == (4, 1, 40) and torch.equal(_bits(short.cpu()), _bits(feats[:4, :1]))


def test_fbank_padded_rejects_on_the_host():
    import sparch_amd as sp
    wave = torch.zeros(3, 1000, device=DEV)
    with pytest.raises(ValueError, match="exceeds"):
        sp.fbank_padded(wave, [400, 1001, 10])
    with pytest.raises(ValueError, match="one frame"):
        sp.fbank_padded(wave, [0, 399, -5])
    with pytest.raises(ValueError):
        sp.fbank_padded(wave, [400, 400])          # one length per clip
    feats, frames = sp.fbank_padded(wave, [-7, 400, 1000])   # a negative length counts as 0
    assert frames.tolist() == [0, 1, 4] and not bool(feats[0].any())


def _read_pcm(path):
    with wave.open(path, "rb") as w:
        return np.frombuffer(w.readframes(w.getnframes()), "<i2").astype(np.float64) / 32768


def test_sc_loader_batch_is_fbank_per_clip_then_pad_sequence(tmp_path):
    import sparch_amd as sp
    from sparch_amd.dataloaders.nonspiking_datasets import load_hd_or_sc
    root = str(tmp_path / "sc")
    lengths = [16000] * 12                  # file k of the tree (word-major, 4 per word) has lengths[k] samples
    lengths[9], lengths[5], lengths[1], lengths[10] = 300, 12345, 15999, 8000   # the first validation batch
    expect = make_sc_tree(root, n_train=1, n_valid=2, n_test=1, lengths=lengths)
    loader = load_hd_or_sc("sc", root, "valid", 4, shuffle=False, device=DEV)
    xs, xlens, ys = next(iter(loader))
    assert xs.is_cuda and xs.dtype == torch.float32
    names = [n for n, _ in expect["validation"][:4]]
    waves = [_read_pcm(os.path.join(root, n)) for n in names]
    assert [len(w) for w in waves] == [300, 12345, 15999, 8000]   # a clip without frames, and T_max < ld
    feats = [torch.from_numpy(fo.fbank(w).astype(np.float32)) if len(w) >= 400 else torch.zeros(0, 40)
             for w in waves]
    ref = torch.nn.utils.rnn.pad_sequence(feats, batch_first=True)
    assert xlens.tolist() == [f.shape[0] for f in feats]
    assert ys.dtype == torch.int64 and ys.tolist() == [y for _, y in expect["validation"][:4]]
    xs = xs.cpu()
    assert xs.shape == ref.shape
    for i, f in enumerate(feats):
        n = f.shape[0]
        assert not bool(xs[i, n:].any())                 # zeros exactly where pad_sequence puts them
        if n:
            _close_to_oracle(xs[i, :n].numpy(), waves[i])
            alone = sp.fbank(torch.from_numpy(waves[i]).float().to(DEV)).cpu()[0]
            assert torch.equal(_bits(xs[i, :n]), _bits(alone))


def _run(tmp_path, name, args):
    import run_exp
    folder = str(tmp_path / name)
    run_exp.main(args + ["--model_type", "RadLIF", "--nb_hiddens", "64", "--batch_size", "4",
                         "--new_exp_folder", folder])
    return folder


def test_run_exp_on_sc_and_hd_trees(tmp_path, caplog, monkeypatch):
    """The reference's command line on dataset files: train, valid and test run to the end, and the best model is
    saved and loaded back.  The reference saves only when the validation accuracy beats the best so far (starting
    at 0), which would make this test hinge on what two short runs learn: here the evaluation reports its real
    numbers except that an accuracy of 0 is raised to 1e-6, so that the first validation always saves."""
    from sparch_amd.exp import Experiment
    evaluate = Experiment._eval_epoch

    def eval_epoch(self, loader, retried=False):
        loss, acc, rate = evaluate(self, loader, retried)
        return loss, max(acc, 1e-6), rate

    monkeypatch.setattr(Experiment, "_eval_epoch", eval_epoch)

    sc = str(tmp_path / "sc")
    make_sc_tree(sc, n_train=6, n_valid=3, n_test=2, lengths=(16000, 14000, 12345, 9000, 16000, 560, 300))
    torch.manual_seed(3)
    with caplog.at_level("INFO"):
        folder = _run(tmp_path, "exp_sc", ["--dataset_name", "sc", "--data_folder", sc, "--nb_epochs", "1"])
    for line in ("Number of examples in sc training set: 18", "Number of examples in sc validation set: 9",
                 "Number of examples in sc testing set: 6", "Epoch 1: train loss=", "Best model saved",
                 "Loading best model, epoch=1", "Test acc="):
        assert line in caplog.text, line
    assert os.path.exists(folder + "/checkpoints/best_model.pth")
    caplog.clear()

    # HD: the test pass runs on the validation split, as in the reference
    hd = str(tmp_path / "hd")
    make_hd_tree(hd, n_train=10, n_test=6, lengths=(16000, 11000, 20000, 7000))
    torch.manual_seed(4)
    with caplog.at_level("INFO"):
        folder = _run(tmp_path, "exp_hd", ["--dataset_name", "hd", "--data_folder", hd, "--nb_epochs", "1"])
    for line in ("Number of examples in hd train set: 10", "Number of examples in hd test set: 6",
                 "Epoch 1: train loss=", "Best model saved", "Loading best model, epoch=1", "Test acc=",
                 "This dataset uses the same split for validation and testing."):
        assert line in caplog.text, line
    assert os.path.exists(folder + "/checkpoints/best_model.pth")
