"""NumPy restatement of the HD / SC training augmentation (torchaudio_augmentations 0.2.4 + sox 14.4 `reverb`, as
DESIGN.md §4 "augment" states it), written sample-sequentially in fp32 with one rounding per operation.  The tests
hold sparch_augment_padded to it bit for bit (noise off).  Nothing here is a test."""
import math

import numpy as np

f32 = np.float32
COMB_LEN = (1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617)
ALLPASS_LEN = (225, 341, 441, 556)
FB_A = -1 / math.log(0.7)
FB_B = 100 / (math.log(0.02) * FB_A + 1)


def feedback(R):
    return f32(1 - math.exp((R - FB_B) / (FB_A * FB_B)))


def damping(D):
    return f32(D / 100 * 0.3 + 0.2)


def delays(S, rate):
    """(combs (2, 8), all-passes (2, 4)) ring sizes of the two filter arrays."""
    scale, r = S / 100 * 0.9 + 0.1, rate / 44100
    combs = np.zeros((2, 8), np.int64)
    aps = np.zeros((2, 4), np.int64)
    for k in range(2):
        for m in range(12):
            o = k * (-1) ** m
            if m < 8:
                combs[k, m] = math.floor(scale * r * (COMB_LEN[m] + 12 * o) + 0.5)
            else:
                aps[k, m - 8] = math.floor(r * (ALLPASS_LEN[m - 8] + 12 * o) + 0.5)
    return combs, aps


def dry(x, polarity, gain, ratio, noise=None):
    """Stages 1-3 on fp32 samples; `noise`: the values stage 2 adds (None: stage off)."""
    v = np.asarray(x, f32).copy()
    if polarity:
        v = -v
    if noise is not None:
        v = (v + np.asarray(noise, f32)).astype(f32)
    if gain:
        v = np.clip(v * f32(ratio), f32(-1), f32(1)).astype(f32)
    return v


def noise_std(x, u, min_snr, max_snr):
    """random.uniform(min_snr * std, max_snr * std) in fp32 (std unbiased, taken in float64)."""
    sd = f32(np.std(np.asarray(x, np.float64), ddof=1))
    a, b = f32(min_snr) * sd, f32(max_snr) * sd
    return f32(a + (b - a) * f32(u))


def reverb(clips, R, D, S, rate=16000):
    """sox `reverb R D S` then `channels 1` (two wet channels, each clipped, averaged) for a list of fp32 clips; each
    clip has its own R, D, S (sequences).  The clips advance together, one sample at a time."""
    n = len(clips)
    if n == 0:
        return []
    T = max(len(c) for c in clips)
    x = np.zeros((n, T), f32)
    for i, c in enumerate(clips):
        x[i, :len(c)] = np.clip(np.asarray(c, f32), f32(-1), f32(1))
    fb = np.array([feedback(float(v)) for v in R], f32)[:, None]
    dp = np.array([damping(float(v)) for v in D], f32)[:, None]
    csz = np.zeros((n, 16), np.int64)
    asz = np.zeros((n, 8), np.int64)
    for i, s in enumerate(S):
        c, a = delays(float(s), rate)
        csz[i], asz[i] = c.reshape(-1), a.reshape(-1)           # index k * 8 + j, k * 4 + j
    cbase = np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(csz, 1)[:, :-1]], 1)
    abase = np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(asz, 1)[:, :-1]], 1)
    cring = np.zeros((n, int(csz.sum(1).max())), f32)
    aring = np.zeros((n, int(asz.sum(1).max())), f32)
    rows16, rows2 = np.arange(n)[:, None].repeat(16, 1), np.arange(n)[:, None].repeat(2, 1)
    store = np.zeros((n, 16), f32)
    out = np.zeros((n, T), f32)
    half, gain = f32(0.5), f32(0.015)
    for t in range(T):
        xt = x[:, t:t + 1]
        slot = cbase + t % csz                                   # the ring holds the last N values: t - N's slot
        y = cring[rows16, slot]
        store = (y + (store - y) * dp).astype(f32)
        cring[rows16, slot] = xt + store * fb
        o = np.zeros((n, 2), f32)
        for j in range(7, -1, -1):
            o = o + y[:, [j, 8 + j]]
        for j in range(3, -1, -1):
            sl = abase[:, [j, 4 + j]] + t % asz[:, [j, 4 + j]]
            ya = aring[rows2, sl]
            aring[rows2, sl] = o + ya * half
            o = ya - o
        wet = o * gain
        out[:, t] = half * (np.clip(xt[:, 0] + wet[:, 0], f32(-1), f32(1))
                            + np.clip(xt[:, 0] + wet[:, 1], f32(-1), f32(1)))
    return [out[i, :len(c)].copy() for i, c in enumerate(clips)]


def augment(clips, params, rate=16000, noise=None):
    """The whole chain on a list of fp32 clips with the table of `draw_augmentation` (noise: per clip the values
    stage 2 adds, or None for the stage off)."""
    vs = [dry(c, p[0] == 1, p[2] == 1, p[5], None if noise is None else noise[i])
          for i, (c, p) in enumerate(zip(clips, params))]
    rev = [i for i, p in enumerate(params) if p[3] == 1]
    outs = reverb([vs[i] for i in rev], [params[i][6] for i in rev], [params[i][7] for i in rev],
                  [params[i][8] for i in rev], rate)
    for i, o in zip(rev, outs):
        vs[i] = o
    return vs
