"""GPU: waveform augmentation on the device (sparch_augment_padded, augment.hip) bit for bit against the NumPy
restatement (tests/augment_numpy.py) with the noise off; the noise stage's statistics; argument checks; the HD / SC
loaders with SPARCH_AUGMENT=restated against the restatement of their host samples; run_exp.py --use_augm 1."""
import os
import random

import numpy as np
import pytest
import torch

from tests import augment_numpy as an
from tests import flac_writer as fw
from tests.audio_trees import clip_pcm, make_hd_tree, make_sc_tree
from tests.kit import DEV

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 39, 40, 41, 399, 400, 12345, 16000]
RDS = [(0, 0, 0), (99, 99, 99), (0, 99, 0), (99, 0, 99)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _raw(wave, lengths, params, seed=0, min_snr=0.0001, max_snr=0.9, rate=16000, out=None):
    """sparch_augment_padded on device tensors, into `out` (default: NaN-filled); returns (status, out)."""
    from sparch_amd._capi import lib, ptr
    n, ld = wave.shape
    if out is None:
        out = torch.full((n, ld), float("nan"), device=DEV)
    lens = torch.as_tensor(lengths, dtype=torch.int32).to(DEV)
    prm = torch.as_tensor(params, dtype=torch.float32).to(DEV)
    st = lib.sparch_augment_padded(n, ld, ptr(lens), 1 if wave.dtype == torch.int16 else 0, ptr(wave), ptr(prm),
                                   min_snr, max_snr, seed, rate, ptr(out), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, out


def _table():
    """Every combination of polarity, gain and reverb (noise off) for every length; R, D, S at 0 and 99."""
    rows, lens = [], []
    for li, n in enumerate(LENGTHS):
        for combo in range(8):
            pol, gain, rev = combo & 1, (combo >> 1) & 1, (combo >> 2) & 1
            r, d, s = RDS[(li + combo) % len(RDS)]
            ratio = np.float32(10 ** ((-20 + 19 * ((li * 8 + combo) % 11) / 10) / 20))
            rows.append([pol, 0, gain, rev, 0, ratio, r, d, s])
            lens.append(n)
    return np.array(rows, np.float32), lens


@pytest.mark.parametrize("rate,dtype", [(8000, "fp32"), (16000, "fp32"), (48000, "fp32"), (16000, "int16")])
def test_bit_equal_to_restatement(rate, dtype):
    import sparch_amd as sp
    params, lens = _table()
    ld = max(lens) + 37
    g = np.random.default_rng(rate + len(dtype))
    if dtype == "int16":
        pcm = g.integers(-32768, 32768, size=(len(lens), ld)).astype(np.int16)
        host = pcm.astype(np.float32) / np.float32(32768)
        wave = torch.from_numpy(pcm).to(DEV)
    else:   # beyond +-1 on purpose: the gain and the reverb clip, polarity alone does not
        host = (g.uniform(-1.6, 1.6, size=(len(lens), ld)) * np.sin(np.arange(ld) / 50.0)).astype(np.float32)
        wave = torch.from_numpy(host).to(DEV)
    st, out = _raw(wave, lens, params, rate=rate)
    assert st == 0
    out = out.cpu()
    ref = an.augment([host[i, :n] for i, n in enumerate(lens)], params, rate)
    for i, n in enumerate(lens):
        got = out[i, :n].numpy()
        assert np.array_equal(got.view(np.int32), ref[i].view(np.int32)), (i, n, params[i].tolist(),
                                                                            np.flatnonzero(got != ref[i])[:5])
        assert torch.isnan(out[i, n:]).all(), (i, n)        # nothing written past the clip
    fresh = sp.augment_padded(wave, lens, params, 0, 0.0001, 0.9, sample_rate=rate).cpu()
    for i, n in enumerate(lens):
        assert torch.equal(_bits(fresh[i, :n]), _bits(out[i, :n]))


def test_noise_statistics():
    B, N, min_snr, max_snr = 256, 16000, 0.0001, 0.9
    g = np.random.default_rng(5)
    t = np.arange(N) / 16000.0
    host = (0.3 * np.sin(2 * np.pi * g.uniform(100, 3000, (B, 1)) * t + g.uniform(0, 6.3, (B, 1)))).astype(np.float32)
    params = np.zeros((B, 9), np.float32)
    params[:, 1] = 1
    params[:, 4] = g.uniform(0.05, 1.0, B)
    wave = torch.from_numpy(host).to(DEV)
    st, out = _raw(wave, [N] * B, params, seed=1234, min_snr=min_snr, max_snr=max_snr)
    assert st == 0
    d = out.cpu().numpy().astype(np.float64) - host
    expect = np.array([an.noise_std(host[i], params[i, 4], min_snr, max_snr) for i in range(B)], np.float64)
    mean, sd = d.mean(1), d.std(1)
    assert (np.abs(mean) <= 5 * expect / np.sqrt(N)).all()
    assert (np.abs(sd / expect - 1) <= 0.03).all(), np.abs(sd / expect - 1).max()
    z = (d - mean[:, None]) / sd[:, None]
    assert np.abs((z[:-1] * z[1:]).mean(1)).max() < 0.05                 # neighbouring rows
    assert np.abs((z[:, :-1] * z[:, 1:]).mean(1)).max() < 0.05           # lag 1
    kurt = (z ** 4).mean(1) - 3
    assert np.abs(kurt).max() <= 0.2, np.abs(kurt).max()
    _, again = _raw(wave, [N] * B, params, seed=1234, min_snr=min_snr, max_snr=max_snr)
    _, other = _raw(wave, [N] * B, params, seed=1235, min_snr=min_snr, max_snr=max_snr)
    assert torch.equal(_bits(again), _bits(out))
    assert not torch.equal(_bits(other), _bits(out))
    # shorter than 2 samples: no noise (the std is undefined)
    st, short = _raw(wave[:2, :4].contiguous(), [1, 0], params[:2])
    assert st == 0 and short[0, 0].item() == host[0, 0] and torch.isnan(short[0, 1:]).all()


def test_invalid_arguments_return_einval():
    import sparch_amd as sp
    from sparch_amd._capi import lib
    wave = torch.zeros(2, 100, device=DEV)
    lens = torch.tensor([100, 50], dtype=torch.int32, device=DEV)
    prm = torch.zeros(2, 9, device=DEV)
    out = torch.full((2, 100), float("nan"), device=DEV)
    p = [x.data_ptr() for x in (lens, wave, prm, out)]
    s = torch.cuda.current_stream().cuda_stream
    call = lib.sparch_augment_padded
    assert call(2, 100, p[0], 0, p[1], p[2], 0.1, 0.9, 1, 16000, p[3], s) == 0
    assert call(-1, 100, p[0], 0, p[1], p[2], 0.1, 0.9, 1, 16000, p[3], s) == -1
    assert call(2, -1, p[0], 0, p[1], p[2], 0.1, 0.9, 1, 16000, p[3], s) == -1
    assert call(2, 100, None, 0, p[1], p[2], 0.1, 0.9, 1, 16000, p[3], s) == -1
    assert call(2, 100, p[0], 0, None, p[2], 0.1, 0.9, 1, 16000, p[3], s) == -1
    assert call(2, 100, p[0], 0, p[1], None, 0.1, 0.9, 1, 16000, p[3], s) == -1
    assert call(2, 100, p[0], 0, p[1], p[2], 0.1, 0.9, 1, 16000, None, s) == -1
    assert call(2, 100, p[0], 2, p[1], p[2], 0.1, 0.9, 1, 16000, p[3], s) == -1
    assert call(2, 100, p[0], 0, p[1], p[2], 0.1, 0.9, 1, 7999, p[3], s) == -1
    assert call(2, 100, p[0], 0, p[1], p[2], 0.1, 0.9, 1, 48001, p[3], s) == -1
    assert call(0, 100, None, 0, None, None, 0.1, 0.9, 1, 16000, None, s) == 0
    assert lib.sparch_augment_lds_bytes(7999) == 0 and lib.sparch_augment_lds_bytes(48000) <= 160 * 1024 - 1024
    torch.cuda.synchronize()
    o = out.cpu()   # the valid call wrote its clips (no stage on: a copy); the others launched nothing
    assert not o[0].isnan().any() and not o[1, :50].isnan().any() and o[1, 50:].isnan().all()
    ok = np.zeros((2, 9), np.float32)
    for bad, col, val in (("flags", 0, 2), ("uniform", 4, 1.5), ("uniform", 4, -0.1), ("100", 6, 101), ("100", 8, -1)):
        t = ok.copy()
        t[1, col] = val
        with pytest.raises(ValueError):
            sp.augment_padded(wave, [100, 50], t, 0, 0.1, 0.9)
    with pytest.raises(ValueError, match="exceeds"):
        sp.augment_padded(wave, [101, 50], ok, 0, 0.1, 0.9)
    with pytest.raises(ValueError):
        sp.augment_padded(wave, [100, 50], ok[:1], 0, 0.1, 0.9)
    with pytest.raises(ValueError, match="sample rate"):
        sp.augment_padded(wave, [100, 50], ok, 0, 0.1, 0.9, sample_rate=96000)


def _seed_with_every_stage_both_ways(n, p_noise):
    """A seed of Python's `random` (which alone decides the stages) under which every stage is applied to some clips
    of an n-clip batch and skipped for others."""
    from sparch_amd.dataloaders.augment import draw_augmentation
    for seed in range(1000):
        random.seed(seed)
        params, _ = draw_augmentation(n, 0.0001, 0.9, p_noise)
        if all(0 < params[:, c].sum() < n for c in (0, 2, 3)):
            return seed
    raise AssertionError("no seed")


def _pad(rows, ld):
    out = np.zeros((len(rows), ld), np.float32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return torch.from_numpy(out).to(DEV)


def _check_loader(monkeypatch, name, root, train_rows):
    """train_rows: the host samples (fp32) of the training split in loader order (shuffle off, one batch)."""
    import sparch_amd as sp
    from sparch_amd.dataloaders import nonspiking_datasets as nsd
    n = len(train_rows)
    monkeypatch.setenv("SPARCH_AUGMENT", "restated")
    drawn, draw = [], nsd.draw_augmentation

    def record(*args):   # the loader's own draws (the DataLoader also takes a torch draw when it starts)
        drawn.append(draw(*args))
        return drawn[-1]

    monkeypatch.setattr(nsd, "draw_augmentation", record)
    random.seed(_seed_with_every_stage_both_ways(n, 0.0))
    torch.manual_seed(1)
    kw = dict(use_augm=True, p_noise=0.0, device=DEV)
    xs, xlens, ys = next(iter(nsd.load_hd_or_sc(name, root, "train", n, shuffle=False, **kw)))
    assert len(drawn) == 1
    params = drawn[0][0]
    for c in (0, 2, 3):                         # polarity, gain and reverb each applied and skipped
        assert 0 < params[:, c].sum() < n
    assert not params[:, 1].any()
    ref_wave = an.augment(train_rows, params, 16000)
    ref, frames = sp.fbank_padded(_pad(ref_wave, max(len(r) for r in train_rows)), [len(r) for r in train_rows])
    assert xlens.tolist() == frames.tolist()
    assert torch.equal(_bits(xs.cpu()), _bits(ref.cpu()))
    plain = next(iter(nsd.load_hd_or_sc(name, root, "train", n, shuffle=False, device=DEV)))[0]
    assert not torch.equal(_bits(plain.cpu()), _bits(xs.cpu()))
    for split in ("valid", "test"):             # not augmented: the batches of use_augm=False
        a = list(nsd.load_hd_or_sc(name, root, split, 3, shuffle=False, **kw))
        b = list(nsd.load_hd_or_sc(name, root, split, 3, shuffle=False, device=DEV))
        assert len(a) == len(b) > 0
        for (xa, la, ya), (xb, lb, yb) in zip(a, b):
            assert torch.equal(_bits(xa.cpu()), _bits(xb.cpu())) and torch.equal(la, lb) and torch.equal(ya, yb)
    assert len(drawn) == 1


def test_sc_loader_with_augmentation(tmp_path, monkeypatch):
    from sparch_amd.dataloaders.audio import read_clip
    root = str(tmp_path / "sc")
    files = make_sc_tree(root, n_train=4, n_valid=2, n_test=2, lengths=(16000, 12345, 9000, 16000, 400, 15999))
    rows = []
    for rel, _ in files["training"]:
        x, _ = read_clip(os.path.join(root, rel))
        rows.append(x.astype(np.float32) / np.float32(32768))
    _check_loader(monkeypatch, "sc", root, rows)


def test_hd_flac_loader_with_augmentation(tmp_path, monkeypatch):
    root = str(tmp_path / "hd")
    lengths = (16000, 11000, 20000, 7000, 16000)
    fw.make_hd_flac_tree(root, n_train=8, n_test=4, lengths=lengths)
    rows = []
    for i in range(8):   # make_hd_flac_tree's samples of the train split, file k = i
        digit = (3 * i + len("train")) % 10
        rows.append(clip_pcm(lengths[i % len(lengths)], 200.0 + 150.0 * digit, 100 + i).astype(np.float32)
                    / np.float32(32768))
    _check_loader(monkeypatch, "hd", root, rows)


def test_run_exp_with_use_augm_on_hd(tmp_path, caplog, monkeypatch):
    import run_exp
    from sparch_amd.exp import Experiment
    evaluate = Experiment._eval_epoch

    def eval_epoch(self, loader, retried=False):   # as test_audio_frontend_gpu: the first validation always saves
        loss, acc, rate = evaluate(self, loader, retried)
        return loss, max(acc, 1e-6), rate

    monkeypatch.setattr(Experiment, "_eval_epoch", eval_epoch)
    monkeypatch.setenv("SPARCH_AUGMENT", "restated")
    hd = str(tmp_path / "hd")
    make_hd_tree(hd, n_train=10, n_test=6, lengths=(16000, 11000, 20000, 7000))
    torch.manual_seed(5)
    random.seed(5)
    with caplog.at_level("INFO"):
        run_exp.main(["--dataset_name", "hd", "--data_folder", hd, "--nb_epochs", "1", "--use_augm", "1",
                      "--model_type", "RadLIF", "--nb_hiddens", "64", "--batch_size", "4",
                      "--new_exp_folder", str(tmp_path / "exp_hd")])
    for line in ("Data augmentation is used", "Epoch 1: train loss=", "Test acc="):
        assert line in caplog.text, line
