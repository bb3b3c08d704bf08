"""
TEST INFRASTRUCTURE ONLY: the augmenting gather-and-bin kernel restated in plain numpy.

Contract (include/sparch_hip.h, `sparch_events_gather_bin_aug`): row b of the (batch, 8) float32 table is
(d, a, c, p, m0, m1, k0, k1).  Event j of the sample in batch row b, stored time t (float16 or float32) and stored
unit u (0xFFFF = the marker of a unit that did not fit), goes through, in this order

    1. u == 0xFFFF                                   -> removed
    2. r = uniform(seed, (b << 32) | j);  r < fp32(p) -> removed      (tests/dropout_numpy.uniforms)
    3. t' = fp32(fp32(a * t) + c),  u' = u + d        (two float32 roundings, no FMA: numpy has none)
    4. m0 <= t' < m1  or  k0 <= u' < k1               -> removed
    5. 6. the survivors (t', u') are binned by the reference's rule (oracle.events_numpy.bin_sample), which drops and
       counts t' < 0, t' >= max_time, u' < 0, u' >= nb_units.

n_dropped = everything removed in 1, 2, 4 plus what bin_sample rejects.  Shares no code with the product.
"""
import numpy as np

from oracle.events_numpy import bin_sample
from tests.dropout_numpy import uniforms

MARKER = 0xFFFF


def stored_units(units):
    """What the store keeps of a unit list: uint16, negative or too large -> 0xFFFF (functional.event_arrays_from_mapping)."""
    u = np.asarray(units).astype(np.int64)
    return np.where((u < 0) | (u > MARKER), MARKER, u)


def augment_sample(times, units, row, seed, b):
    """(t' float32, u' int64) of the events that survive steps 1-4, and the number removed."""
    t = np.asarray(times)
    assert t.dtype in (np.float16, np.float32)
    u = stored_units(units)
    d, a, c, p, m0, m1, k0, k1 = (np.float32(v) for v in np.asarray(row, np.float32))
    gone = u == MARKER
    gone |= uniforms(seed, len(t), first_index=int(b) << 32) < p
    tp = (a * t.astype(np.float32)).astype(np.float32) + c          # float32 * float32 -> float32, then + float32
    assert tp.dtype == np.float32
    up = u + int(d)
    gone |= (tp >= m0) & (tp < m1)
    gone |= (up >= int(k0)) & (up < int(k1))
    return tp[~gone], up[~gone], int(gone.sum())


def bin_batch_augmented(samples, idx, table, seed, nb_steps, nb_units, max_time):
    """((B, nb_steps, nb_units) float32 counts, n_dropped) of the batch `idx` over `samples` [(times, units), ...]."""
    out = np.zeros((len(idx), nb_steps, nb_units), np.float32)
    lost = 0
    for b, s in enumerate(idx):
        tp, up, removed = augment_sample(samples[s][0], samples[s][1], table[b], seed, b)
        out[b], rejected = bin_sample(tp, up, nb_steps, nb_units, max_time)
        lost += removed + rejected
    return out, lost
