"""CPU: the host draws of the HD / SC augmentation (sparch_amd.dataloaders.augment) against a stand-in of the
library's draw code, the restatement's delay table and impulse response (tests/augment_numpy.py), and the
SPARCH_AUGMENT opt-in of the loaders."""
import random

import numpy as np
import pytest
import torch

from tests import augment_numpy as an
from tests.audio_trees import make_hd_tree, make_sc_tree


# ---- stand-in: torchaudio_augmentations 0.2.4's draw code, per clip (values recorded instead of applied)
class RandomApply:
    def __init__(self, transforms, p=0.5):
        self.transforms, self.p = transforms, p

    def __call__(self, rec):
        if self.p < random.random():
            return rec
        for t in self.transforms:
            rec = t(rec)
        return rec


class ComposeMany:
    def __init__(self, transforms, num_augmented_samples):
        self.transforms, self.num_augmented_samples = transforms, num_augmented_samples

    def __call__(self, rec):
        for _ in range(self.num_augmented_samples):
            for t in self.transforms:
                rec = t(rec)
        return rec


class PolarityInversion:
    def __call__(self, rec):
        rec[0] = 1
        return rec


class Noise:
    def __init__(self, min_snr=0.0001, max_snr=0.01):
        self.min_snr, self.max_snr = min_snr, max_snr

    def __call__(self, rec):
        rec[1] = 1
        rec[4] = random.uniform(0.0, 1.0)   # random.uniform(min_snr * std, max_snr * std): one random.random()
        return rec


class Gain:
    def __init__(self, min_gain=-20.0, max_gain=-1):
        self.min_gain, self.max_gain = min_gain, max_gain

    def __call__(self, rec):
        rec[2] = 1
        rec[5] = 10 ** (random.uniform(self.min_gain, self.max_gain) / 20)
        return rec


class Reverb:
    def __call__(self, rec):
        rec[3] = 1
        rec[6] = torch.randint(0, 100, size=(1,)).item()
        rec[7] = torch.randint(0, 100, size=(1,)).item()
        rec[8] = torch.randint(0, 100, size=(1,)).item()
        return rec


def _reference_table(n, min_snr, max_snr, p_noise):
    transf = ComposeMany([RandomApply([PolarityInversion()], p=0.8), RandomApply([Noise(min_snr, max_snr)], p_noise),
                          RandomApply([Gain()], p=0.3), RandomApply([Reverb()], p=0.6)], num_augmented_samples=1)
    table = np.zeros((n, 9), np.float32)
    for i in range(n):
        table[i] = transf([0.0] * 9)
    return table


@pytest.mark.parametrize("n", [1, 7, 256])
@pytest.mark.parametrize("p_noise", [0.0, 0.1, 1.0])
def test_draws_match_the_library_per_clip(n, p_noise):
    from sparch_amd.dataloaders.augment import draw_augmentation
    for seed in (0, 12345):
        random.seed(seed)
        torch.manual_seed(seed + 1)
        ref = _reference_table(n, 0.0001, 0.9, p_noise)
        ref_state = (random.getstate(), torch.get_rng_state())
        random.seed(seed)
        torch.manual_seed(seed + 1)
        np.random.seed(seed + 2)
        params, noise_seed = draw_augmentation(n, 0.0001, 0.9, p_noise)
        assert params.dtype == np.float32 and params.shape == (n, 9)
        assert np.array_equal(params, ref)
        assert random.getstate() == ref_state[0]
        assert torch.equal(torch.get_rng_state(), ref_state[1])
        np.random.seed(seed + 2)
        assert draw_augmentation(n, 0.0001, 0.9, p_noise)[1] == noise_seed   # numpy's global generator pins it
    if n == 256:   # every stage both applied and skipped
        for col in range(4 if p_noise == 0.1 else 1):
            assert 0 < params[:, col].sum() < n
    if p_noise == 0.0:
        assert not params[:, 1].any()


def test_delay_table_feedback_and_damping():
    combs, aps = an.delays(0, 16000)
    assert combs.tolist() == [[40, 43, 46, 49, 52, 54, 56, 59], [41, 43, 47, 49, 52, 54, 57, 58]]
    assert aps.tolist() == [[82, 124, 160, 202], [86, 119, 164, 197]]
    for S in (50, 99):
        c, a = an.delays(S, 16000)
        assert np.array_equal(a, aps)                           # the all-passes do not scale with the room
        assert (c > combs).all()
    assert an.delays(50, 16000)[0][0].tolist() == [223, 237, 255, 271, 284, 298, 311, 323]
    assert an.delays(99, 16000)[0][1].tolist() == [406, 423, 463, 483, 516, 532, 564, 577]
    assert an.feedback(0) == np.float32(0.3)
    assert abs(float(an.feedback(99)) - 0.97928) <= 1e-5
    assert an.damping(0) == np.float32(0.2) and an.damping(100) == np.float32(0.5)


def test_impulse_response_at_room_scale_zero():
    x = np.zeros(300, np.float32)
    x[0] = 1
    y = an.reverb([x], [50], [50], [0])[0]
    assert y.dtype == np.float32 and len(y) == 300
    assert y[0] == 1                                           # dry
    assert not y[1:40].any()                                   # exact zeros before the shortest comb
    half_wet = np.float32(0.5) * np.float32(0.015)             # one array's first comb through four all-passes
    assert y[40] == half_wet and y[41] == half_wet
    assert abs(float(y[40]) - 0.0075) < 1e-9


def test_dry_stages_and_clipping():
    x = np.array([0.5, -2.0, 1.5, 0.25], np.float32)
    assert np.array_equal(an.dry(x, True, False, 1.0), -x)     # no clamp without gain
    g = np.float32(10 ** (-6 / 20))
    assert np.array_equal(an.dry(x, False, True, g), np.clip(x * g, -1, 1))
    out = an.reverb([x], [0], [0], [0])[0]                     # input clipped to [-1, 1] before the reverb
    assert np.array_equal(out, np.clip(x, -1, 1))


def test_augmentation_opt_in(tmp_path, monkeypatch):
    from sparch_amd.dataloaders.nonspiking_datasets import load_hd_or_sc
    sc, hd = str(tmp_path / "sc"), str(tmp_path / "hd")
    make_sc_tree(sc)
    make_hd_tree(hd, n_train=2, n_test=2)
    monkeypatch.delenv("SPARCH_AUGMENT", raising=False)
    with pytest.raises(NotImplementedError, match="torchaudio_augmentations"):
        load_hd_or_sc("sc", sc, "train", 2, use_augm=True, device="cpu")
    monkeypatch.setenv("SPARCH_AUGMENT", "")
    with pytest.raises(NotImplementedError, match="SPARCH_AUGMENT"):
        load_hd_or_sc("hd", hd, "train", 2, use_augm=True, device="cpu")
    monkeypatch.setenv("SPARCH_AUGMENT", "sox")
    with pytest.raises(ValueError, match="restated"):
        load_hd_or_sc("sc", sc, "train", 2, use_augm=True, device="cpu")
    monkeypatch.setenv("SPARCH_AUGMENT", "restated")
    for name, root in (("sc", sc), ("hd", hd)):
        loaders = {s: load_hd_or_sc(name, root, s, 2, use_augm=True, device="cpu", min_snr=0.01, max_snr=0.5,
                                    p_noise=0.25)
                   for s in ("train", "valid", "test")}
        assert loaders["train"].dataset.augment == (0.01, 0.5, 0.25)
        assert loaders["valid"].dataset.augment is None and loaders["test"].dataset.augment is None
        assert load_hd_or_sc(name, root, "train", 2, device="cpu").dataset.augment is None
