"""
Host draws of the reference's HD / SC training augmentation (nonspiking_datasets.py:71-78, 170-177):

    ComposeMany([RandomApply([PolarityInversion()], p=0.8), RandomApply([Noise(min_snr, max_snr)], p_noise),
                 RandomApply([Gain()], p=0.3), RandomApply([Reverb(sample_rate=16000)], p=0.6)],
                num_augmented_samples=1)

applied per clip in batch order.  `draw_augmentation` consumes Python's `random` and torch's global CPU generator
exactly as torchaudio_augmentations 0.2.4 does for those clips, and returns the decisions and values as one table
row per clip for `functional.augment_padded`, which applies them to the whole batch on the device:

  * RandomApply(p): r = random.random(); the stage is skipped when p < r;
  * Noise: noise_std = random.uniform(min_snr std, max_snr std) = a + (b - a) random.random(): the table keeps that
    uniform (the std is the device's); the noise itself comes from the device's generator, keyed by `noise_seed`, one
    draw per batch from numpy's global generator (the reference draws the values from numpy);
  * Gain: g = random.uniform(-20, -1) dB, kept as the fp32 ratio 10^(g/20) (torchaudio's Vol multiplies by it);
  * Reverb: reverberance, HF damping, room scale = three torch.randint(0, 100, (1,)) per clip.  They are drawn here
    with ONE torch.randint(0, 100, (3k,)) for the k clips of the batch with reverb: the same values and the same end
    state of the generator as 3k single draws (the stream is one value per element, in order), without 3k calls.
"""
import random

import numpy as np
import torch

AUGM_FIELDS = 9  # SPARCH_AUGM_FIELDS: flags (polarity, noise, gain, reverb), noise uniform, gain ratio, R, D, S
P_POLARITY, P_GAIN, P_REVERB = 0.8, 0.3, 0.6
GAIN_DB = (-20.0, -1)


def draw_augmentation(n_clips, min_snr, max_snr, p_noise):
    """(params (n_clips, AUGM_FIELDS) float32 numpy table, noise_seed int) for one batch.  min_snr / max_snr are not
    drawn from: they enter on the device with the clip's standard deviation (kept in the signature with the
    reference's Noise arguments)."""
    params = np.zeros((n_clips, AUGM_FIELDS), np.float32)
    reverb = []
    for i in range(n_clips):
        row = params[i]
        if not P_POLARITY < random.random():
            row[0] = 1
        if not p_noise < random.random():
            row[1] = 1
            row[4] = random.random()            # random.uniform(min_snr * std, max_snr * std)
        if not P_GAIN < random.random():
            row[2] = 1
            row[5] = 10 ** (random.uniform(*GAIN_DB) / 20)
        if not P_REVERB < random.random():
            row[3] = 1
            reverb.append(i)
    if reverb:
        params[reverb, 6:9] = torch.randint(0, 100, (3 * len(reverb),)).numpy().reshape(-1, 3)
    noise_seed = int(np.random.randint(0, np.iinfo(np.int64).max, dtype=np.int64))
    return params, noise_seed
