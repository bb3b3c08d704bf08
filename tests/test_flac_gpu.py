"""GPU: FLAC decoding on the device (sparch_flac_decode_padded, flac.hip) against the samples the test encoder
(tests/flac_writer.py) was given, exactly; corrupt and truncated files; the HD loader on FLAC trees against the same
trees in WAV; the STREAMINFO MD5 check; run_exp.py on an HD tree of FLAC files."""
import os

import numpy as np
import pytest
import torch

from tests import flac_writer as fw
from tests.audio_trees import clip_pcm, make_hd_tree
from tests.kit import DEV

pytestmark = pytest.mark.gpu


def _signal(n, bps, channels=1, seed=0, noise=0.02):
    """Tones plus a little noise at full scale of `bps` bits, (n, channels) int64."""
    g = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    cols = []
    for c in range(channels):
        x = 0.5 * np.sin(2 * np.pi * (300.0 + 211.0 * c) * t + c) + noise * g.uniform(-1, 1, n)
        cols.append(np.clip(np.round(x * (2 ** (bps - 1) - 1)), -(2 ** (bps - 1)), 2 ** (bps - 1) - 1))
    return np.stack(cols, 1).astype(np.int64)


def _roundtrip(tmp_path, x, bps, rate=16000, **kw):
    from sparch_amd.dataloaders.audio import read_audio
    path = str(tmp_path / "clip.flac")
    fw.write_flac(path, x, bps, rate, **kw)
    y, r = read_audio(path)
    assert r == rate
    x0 = np.asarray(x).reshape(len(x), -1)[:, 0]
    if bps == 16 and np.asarray(x).reshape(len(x), -1).shape[1] == 1:
        assert y.dtype == np.int16
        assert np.array_equal(y, x0.astype(np.int16))
    else:
        assert y.dtype == np.float32
        assert np.array_equal(y, (x0 * 2.0 ** -(bps - 1)).astype(np.float32))


@pytest.mark.parametrize("bps", [8, 12, 16, 20, 24])
def test_bits_per_sample(tmp_path, bps):
    _roundtrip(tmp_path, _signal(10000, bps, seed=bps), bps, blocks=4096)


def test_every_lpc_order_precision_and_shift(tmp_path):
    """Frame f: LPC order f + 1 (1-32), precision 1 + f % 15, shift f % 16 (coefficients clipped to the
    precision), partition order f % 9 (lowered where the block does not split)."""
    def plan(f, c, x):
        return dict(kind="lpc", order=f + 1, precision=1 + f % 15, shift=f % 16, porder=f % 9)
    _roundtrip(tmp_path, _signal(32 * 512, 16, seed=1), 16, blocks=512, plan=plan)


def test_fixed_constant_verbatim_and_wasted_bits(tmp_path):
    x = _signal(12 * 256, 16, seed=2)
    x[256:512] = 1234                                 # frame 1: constant
    x[512:768] = -7
    x[768:1024] &= ~np.int64(7)                       # frame 3: 3 wasted bits
    x[1024:1280] = (x[1024:1280] >> 5) << 5           # frame 4: 5 wasted bits

    def plan(f, c, x):
        if f in (1, 2):
            return dict(kind="constant")
        if f == 5:
            return dict(kind="verbatim")
        if f == 6:
            return dict(kind="verbatim", wasted=0)
        if f >= 7:
            return dict(kind="fixed", order=f - 7, porder=2)
        return dict(kind="lpc", order=4)
    _roundtrip(tmp_path, x, 16, blocks=256, plan=plan)


def test_residual_methods_partitions_and_escapes(tmp_path):
    x = _signal(18 * 512, 20, seed=3, noise=0.3)
    x[9 * 512 + 64:9 * 512 + 300] = 0               # a run of zeros: escaped partitions of width 0
    x[5 * 512:6 * 512] //= 1 << 13                    # quiet frame 5: Rice parameter 0, unary codes of ~100 bits

    def plan(f, c, x):
        spec = dict(kind="fixed" if f % 2 else "lpc", order=2, porder=f % 9, method=f % 2)
        if f in (3, 9, 10):
            spec["escape"] = "all"
        elif f == 4:
            spec["escape"] = (0, 2)
        elif f == 5:
            spec["params"] = [0] * 32                 # long unary codes (method 1: 5-bit parameter 0)
        return spec
    _roundtrip(tmp_path, x, 20, blocks=512, plan=plan)
    y = x.copy()
    y[:] = 0
    _roundtrip(tmp_path, y, 16, blocks=512, plan=lambda f, c, x: dict(kind="lpc", order=3, escape="all"))


@pytest.mark.parametrize("assignment", ["independent", "left_side", "side_right", "mid_side"])
@pytest.mark.parametrize("bps", [16, 24])
def test_channel_assignments(tmp_path, assignment, bps):
    x = _signal(9000, bps, channels=2, seed=4)
    x[:, 1] = -x[:, 0] // 3 + x[:, 1] // 2
    _roundtrip(tmp_path, x, bps, blocks=1152, assignment=assignment,
               plan=lambda f, c, b: dict(kind="lpc" if f % 2 else "fixed", order=6 if f % 2 else 2, porder=3))


def test_decorrelation_per_frame_and_many_channels(tmp_path):
    modes = ["independent", "left_side", "side_right", "mid_side"]
    x = _signal(4 * 1000 + 333, 16, channels=2, seed=5)
    _roundtrip(tmp_path, x, 16, blocks=1000, assignment=lambda f: modes[f % 4])
    for ch in (3, 8):
        _roundtrip(tmp_path, _signal(3000, 12, channels=ch, seed=ch), 12, blocks=1024)


@pytest.mark.parametrize("bs", [192, 576, 1152, 2304, 4608, 100, 256, 1000, 512, 1024, 2048, 4096, 8192, 16384,
                                32768, 65535])
def test_block_size_codes_fixed_blocking(tmp_path, bs):
    n = bs * 2 + bs // 3 + 1                          # a short last frame
    _roundtrip(tmp_path, _signal(n, 16, seed=bs), 16, blocks=bs)


def test_variable_blocking_every_block_size_code(tmp_path):
    sizes = [192, 576, 1152, 2304, 4608, 100, 1000, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 17, 40]
    _roundtrip(tmp_path, _signal(sum(sizes), 16, seed=6), 16, blocks=sizes, variable=True)
    _roundtrip(tmp_path, _signal(sum(sizes), 24, seed=7), 24, blocks=sizes, variable=True, bs_code=7)


@pytest.mark.parametrize("rate,sr_code", [(r, c) for r, c in fw.RATES.items()] +
                         [(11000, 12), (22051, 13), (50000, 14), (16000, 0), (12345, 13)])
def test_sample_rate_codes(tmp_path, rate, sr_code):
    _roundtrip(tmp_path, _signal(3000, 16, seed=rate), 16, rate=rate, blocks=1024, sr_code=sr_code)


def test_sample_size_from_streaminfo(tmp_path):
    _roundtrip(tmp_path, _signal(3000, 20, seed=8), 20, blocks=1024, ss_code=0)


def _planted(n_frames=6, bs=1024, target=3):
    """A 16-bit mono stream whose frame `target` - 1 is verbatim and carries, inside its samples, a valid header
    (CRC-8 included) of frame `target`: the scan takes it for frame `target`, the chain check must repair."""
    x = _signal(n_frames * bs, 16, seed=9)
    head = fw.frame_header(bs, target, False, 0, 16, 16000)
    head += bytes([fw.crc8(head)])
    head += b"\x00" * (len(head) % 2)
    j = (target - 1) * bs + 100                       # verbatim 16-bit samples are byte-aligned big-endian pairs
    for k in range(len(head) // 2):
        x[j + k, 0] = int.from_bytes(head[2 * k:2 * k + 2], "big", signed=True)
    plan = lambda f, c, b: dict(kind="verbatim", wasted=0) if f == target - 1 else dict(kind="lpc", order=8)
    return x, plan, head


def test_false_frame_header_is_repaired(tmp_path):
    x, plan, head = _planted()
    data = fw.encode_flac(x, 16, 16000, blocks=1024, plan=plan)
    assert data.count(head[:-1] if len(head) % 2 else head) >= 1   # the planted header is in the file
    _roundtrip(tmp_path, x, 16, blocks=1024, plan=plan)
    # and in a batch next to clean clips, through the loader's entry point
    import sparch_amd as sp
    from sparch_amd.dataloaders.audio import parse_flac
    clean = [fw.encode_flac(_signal(3000 + 500 * k, 16, seed=20 + k), 16, 16000, blocks=1024) for k in range(3)]
    streams = [clean[0], data, clean[1], clean[2]]
    wave = torch.full((4, 6144), -1, dtype=torch.int16, device=DEV)
    err = sp.flac_decode_padded(streams, [parse_flac(s) for s in streams], wave)
    assert err.cpu().tolist()[0] == 0
    assert np.array_equal(wave[1].cpu().numpy(), x[:, 0].astype(np.int16))


def _decode_rows(streams, ld, dtype, fill):
    import sparch_amd as sp
    from sparch_amd.dataloaders.audio import parse_flac
    infos = [parse_flac(s) for s in streams]
    wave = torch.full((len(streams) + 1, ld), fill, dtype=dtype, device=DEV)
    err = sp.flac_decode_padded(streams, infos, wave, rows=list(range(1, len(streams) + 1)))
    return wave.cpu(), err.cpu(), infos


@pytest.mark.parametrize("damage", ["corrupt", "truncate"])
def test_corrupt_and_truncated_files_raise_and_stay_in_their_rows(tmp_path, damage):
    from sparch_amd.dataloaders.audio import FlacError, read_audio
    from sparch_amd.functional import flac_error_message
    x = _signal(5000, 16, seed=10)
    good = fw.encode_flac(x, 16, 16000, blocks=1024)
    first = fw.first_frame_offset(good)
    bad = bytearray(good)
    if damage == "corrupt":
        bad[first + (len(good) - first) // 2] ^= 0x10
    else:
        bad = bad[:len(good) - 700]
    bad = bytes(bad)
    path = str(tmp_path / f"{damage}.flac")
    with open(path, "wb") as f:
        f.write(bad)
    with pytest.raises(FlacError) as e:
        read_audio(path)
    assert path in str(e.value)

    # in a batch: the error names the damaged clip; nothing outside each clip's own samples is written
    for dtype, fill in ((torch.int16, 12345), (torch.float32, float("nan"))):
        wave, err, infos = _decode_rows([good, bad, good], 6000, dtype, fill)
        msg = flac_error_message(err, ["a.flac", path, "c.flac"])
        assert msg and msg.startswith(path), msg
        assert int(err[0]) == 1
        ref = torch.from_numpy(x[:, 0].astype(np.int16)) if dtype == torch.int16 else \
            torch.from_numpy((x[:, 0] * 2.0 ** -15).astype(np.float32))
        for r in (1, 3):
            assert torch.equal(wave[r, :5000], ref)
        untouched = torch.full((6000,), fill, dtype=dtype)
        for r, n in ((0, 0), (1, 5000), (2, 5000), (3, 5000)):
            tail, want = wave[r, n:], untouched[n:]
            assert torch.equal(tail.view(torch.int16) if dtype == torch.int16 else tail.view(torch.int32),
                               want.view(torch.int16) if dtype == torch.int16 else want.view(torch.int32)), r


def test_bad_crc8_and_crc16_are_errors(tmp_path):
    from sparch_amd.functional import flac_error_message
    x = _signal(5000, 16, seed=11)
    streams = [fw.encode_flac(x, 16, 16000, blocks=1024, bad_crc16=[2]),
               fw.encode_flac(x, 16, 16000, blocks=1024, bad_crc8=[3])]
    for s in streams:
        _, err, _ = _decode_rows([s], 5000, torch.int16, 0)
        assert flac_error_message(err, ["x.flac"]), "a frame with a wrong CRC decoded without error"


def _batches(loader):
    return [(xs.cpu(), xl.clone(), ys.clone()) for xs, xl, ys in loader]


def test_hd_loader_flac_equals_wav_and_mixed(tmp_path):
    from sparch_amd.dataloaders.nonspiking_datasets import load_hd_or_sc
    lengths = (16000, 11000, 20000, 7000, 300, 4097)
    args = dict(n_train=10, n_test=3, lengths=lengths)
    make_hd_tree(str(tmp_path / "wav"), **args)
    fw.make_hd_flac_tree(str(tmp_path / "flac"), **args)
    fw.make_hd_flac_tree(str(tmp_path / "mixed"), flac_every=2, **args)
    ref = _batches(load_hd_or_sc("hd", str(tmp_path / "wav"), "train", 4, shuffle=False, device=DEV))
    for tree in ("flac", "mixed"):
        got = _batches(load_hd_or_sc("hd", str(tmp_path / tree), "train", 4, shuffle=False, device=DEV))
        assert len(got) == len(ref) == 3
        for (xa, la, ya), (xb, lb, yb) in zip(got, ref):
            assert torch.equal(la, lb) and torch.equal(ya, yb)
            assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)), tree


def test_hd_loader_24_bit_flac_matches_float_wav(tmp_path):
    """A 24-bit FLAC clip makes the batch fp32: x * 2^-23, the same features as the float WAV of those values."""
    from sparch_amd.dataloaders.nonspiking_datasets import load_hd_or_sc
    from tests.audio_trees import write_raw_wav
    root_f, root_w = tmp_path / "f", tmp_path / "w"
    for root in (root_f, root_w):
        os.makedirs(root / "audio")
    names = []
    for k in range(3):
        x = _signal(9000 + 1000 * k, 24, seed=30 + k)[:, 0]
        stem = f"lang-english_speaker-0{k}_trial-0_digit-{k}"
        fw.write_flac(str(root_f / "audio" / (stem + ".flac")), x, 24, 16000, blocks=4096)
        write_raw_wav(str(root_w / "audio" / (stem + ".wav")), (x * 2.0 ** -23).astype(np.float32), 3, 32)
        names.append(stem)
    for root, ext in ((root_f, ".flac"), (root_w, ".wav")):
        (root / "train_filenames.txt").write_text("".join(n + ext + "\n" for n in names))
    a = _batches(load_hd_or_sc("hd", str(root_f), "train", 3, shuffle=False, device=DEV))
    b = _batches(load_hd_or_sc("hd", str(root_w), "train", 3, shuffle=False, device=DEV))
    assert torch.equal(a[0][0].view(torch.int32), b[0][0].view(torch.int32)) and torch.equal(a[0][1], b[0][1])


def test_streaminfo_md5_checked_on_the_first_batch(tmp_path):
    from sparch_amd.dataloaders.audio import FlacError
    from sparch_amd.dataloaders.nonspiking_datasets import load_hd_or_sc
    fw.make_hd_flac_tree(str(tmp_path / "bad"), n_train=4, n_test=1, md5=b"\x01" * 16)
    with pytest.raises(FlacError, match="MD5") as e:
        next(iter(load_hd_or_sc("hd", str(tmp_path / "bad"), "train", 4, shuffle=False, device=DEV)))
    assert "lang-" in str(e.value) and ".flac" in str(e.value)
    fw.make_hd_flac_tree(str(tmp_path / "zero"), n_train=4, n_test=1, md5=False)   # MD5 0: not checked
    assert len(_batches(load_hd_or_sc("hd", str(tmp_path / "zero"), "train", 2, shuffle=False, device=DEV))) == 2


def test_decode_error_of_a_later_batch_raises_by_the_end_of_the_epoch(tmp_path):
    from sparch_amd.dataloaders.audio import FlacError
    from sparch_amd.dataloaders.nonspiking_datasets import load_hd_or_sc
    root = str(tmp_path / "hd")
    expect = fw.make_hd_flac_tree(root, n_train=6, n_test=1)
    victim = os.path.join(root, "audio", expect["train"][4][0])       # second batch of 2, third batch of ...
    data = bytearray(open(victim, "rb").read())
    data[len(data) // 2] ^= 0x01
    open(victim, "wb").write(bytes(data))
    loader = load_hd_or_sc("hd", root, "train", 2, shuffle=False, device=DEV)
    with pytest.raises(FlacError) as e:
        for _ in loader:
            pass
    assert victim in str(e.value)


def test_run_exp_on_a_flac_hd_tree(tmp_path, caplog, monkeypatch):
    import run_exp
    from sparch_amd.exp import Experiment
    evaluate = Experiment._eval_epoch

    def eval_epoch(self, loader, retried=False):  # as test_audio_frontend_gpu: the first validation always saves
        loss, acc, rate = evaluate(self, loader, retried)
        return loss, max(acc, 1e-6), rate

    monkeypatch.setattr(Experiment, "_eval_epoch", eval_epoch)
    hd = str(tmp_path / "hd")
    fw.make_hd_flac_tree(hd, n_train=10, n_test=6, lengths=(16000, 11000, 20000, 7000))
    torch.manual_seed(4)
    folder = str(tmp_path / "exp_hd")
    with caplog.at_level("INFO"):
        run_exp.main(["--dataset_name", "hd", "--data_folder", hd, "--nb_epochs", "1", "--model_type", "RadLIF",
                      "--nb_hiddens", "64", "--batch_size", "4", "--new_exp_folder", folder])
    for line in ("Number of examples in hd train set: 10", "Epoch 1: train loss=", "Best model saved", "Test acc="):
        assert line in caplog.text, line
    assert os.path.exists(folder + "/checkpoints/best_model.pth")
