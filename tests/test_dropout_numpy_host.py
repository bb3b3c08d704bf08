"""
Host tests of tests/dropout_numpy.py, the numpy restatement of the in-kernel dropout mask (no GPU needed).  The
GPU tests (tests/test_dropout_rate_backward_gpu.py) pin the restatement to the kernels; these check that it is
a usable mask at all: deterministic, the right kept share, decorrelated across seeds and layers, and that the
high halves of the 64-bit seed and index take part.
"""
import math

import numpy as np
import pytest

from tests import dropout_numpy as dn

N = 21120  # (11, 15, 128): the element count the shares below are stated for


def _band(n, q):
    """5-sigma half-width of a share estimated from n Bernoulli(q) draws, plus the 2^-24 grid of the uniform."""
    return 5.0 * math.sqrt(q * (1.0 - q) / n) + 2.0 ** -24


def test_mask_is_deterministic_and_two_valued():
    a = dn.keep_mask(1234567, (11, 15, 128), 0.25)
    b = dn.keep_mask(1234567, (11, 15, 128), 0.25)
    assert a.dtype == np.float32 and a.shape == (11, 15, 128)
    np.testing.assert_array_equal(a, b)
    k = np.float32(1.0) / (np.float32(1.0) - np.float32(0.25))
    assert set(np.unique(a).tolist()) == {0.0, float(k)}
    # the flat element index is the C-order position: a reshaped request is the same stream
    np.testing.assert_array_equal(a.reshape(-1), dn.keep_mask(1234567, (N,), 0.25))
    # ... and first_index continues it
    np.testing.assert_array_equal(a.reshape(-1)[1000:], dn.keep_mask(1234567, (N - 1000,), 0.25, first_index=1000))


@pytest.mark.parametrize("p", [0.1, 0.2, 0.25, 0.3, 0.5])
@pytest.mark.parametrize("seed", [0, 1234567, (1 << 62) + 12345, 0x7FFFFFFFFFFFFFFF])
def test_kept_share_within_the_binomial_band(p, seed):
    m = dn.keep_mask(seed, (N,), p)
    share = float((m > 0).mean())
    assert abs(share - (1.0 - p)) <= _band(N, 1.0 - p), (share, 1.0 - p, _band(N, 1.0 - p))


def test_uniforms_are_24_bit_and_flat():
    u = dn.uniforms(99, 1 << 16)
    assert u.dtype == np.float32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    np.testing.assert_array_equal(u * np.float32(16777216.0), np.round(u * np.float32(16777216.0)))
    hist = np.histogram(u, bins=16, range=(0.0, 1.0))[0] / u.size
    assert float(np.abs(hist - 1.0 / 16).max()) <= _band(u.size, 1.0 / 16)


def test_p_zero_keeps_all_with_scale_one():
    m = dn.keep_mask(5, (7, 9, 12), 0.0)
    np.testing.assert_array_equal(m, np.ones((7, 9, 12), np.float32))


def _agreement(a, b):
    return float(((a > 0) == (b > 0)).mean())


def test_seeds_and_layers_decorrelate():
    """Two independent masks with kept share q agree on a share q^2 + (1-q)^2 of the elements (0.5 at p = 0.5)."""
    p, q = 0.5, 0.5
    expect = q * q + (1 - q) * (1 - q)
    base = dn.keep_mask(1234567, (N,), p)
    # the next step's seed, a seed that differs in the high word only, and two layers' seeds as the eager and the
    # captured step form them (a multiple of 0x100000001B3 resp. of 7919 apart)
    others = [1234568, 1234567 + (1 << 32), 1234567 + (1 << 63), 1234567 + 0x100000001B3, 1234567 + 7919]
    for s in others:
        agree = _agreement(base, dn.keep_mask(s, (N,), p))
        assert abs(agree - expect) <= _band(N, expect), (s, agree)
    # a shifted window of the same stream (what a wrong time or feature offset would read)
    for shift in (1, 4, 128, 128 * 15):
        agree = _agreement(base, dn.keep_mask(1234567, (N,), p, first_index=shift))
        assert abs(agree - expect) <= _band(N, expect), (shift, agree)


def test_index_range_across_2_to_the_32_uses_the_high_word():
    p, expect = 0.5, 0.5
    lo = dn.keep_mask(77, (N,), p, first_index=0)
    hi = dn.keep_mask(77, (N,), p, first_index=1 << 32)  # same low 32 bits of every index, high word 1
    assert abs(_agreement(lo, hi) - expect) <= _band(N, expect)
    # a range that crosses the boundary: continuous with its two halves
    first = (1 << 32) - 1000
    cross = dn.keep_mask(77, (N,), p, first_index=first)
    np.testing.assert_array_equal(cross[:1000], dn.keep_mask(77, (1000,), p, first_index=first))
    np.testing.assert_array_equal(cross[1000:], dn.keep_mask(77, (N - 1000,), p, first_index=1 << 32))
    below = dn.keep_mask(77, (N - 1000,), p, first_index=0)  # the same low words without the high one
    assert abs(_agreement(cross[1000:], below) - expect) <= _band(N - 1000, expect)


def test_known_answers_of_the_hash():
    """lowbias32 by hand: mix32(0) = 0, so seed 0 / index 0 gives u = 0 (dropped for any p > 0, kept at p = 0);
    and one value worked with Python integers."""
    assert float(dn.uniforms(0, 1)[0]) == 0.0
    assert float(dn.keep_mask(0, (1,), 0.1)[0]) == 0.0

    def mix(x):
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        x ^= x >> 16
        return x

    seed, idx = 0x123456789ABCDEF0, (5 << 32) + 17
    a = mix((idx & 0xFFFFFFFF) ^ (seed & 0xFFFFFFFF))
    b = mix((a + (idx >> 32) * 0x9E3779B9 + (seed >> 32)) & 0xFFFFFFFF)
    assert float(dn.uniforms(seed, 1, first_index=idx)[0]) == (b >> 8) / 16777216.0


def test_padded_mask_is_the_padded_tensors_mask_sliced():
    B, T, dirs, H, Hp = 3, 5, 2, 7, 8
    m = dn.keep_mask_padded(42, B, T, dirs, H, Hp, 0.25)
    full = dn.keep_mask(42, (B, T, dirs * Hp), 0.25)
    assert m.shape == (B, T, dirs * H)
    np.testing.assert_array_equal(m[..., :H], full[..., :H])
    np.testing.assert_array_equal(m[..., H:], full[..., Hp:Hp + H])
    # and it is NOT the unpadded tensor's mask
    assert not np.array_equal(m, dn.keep_mask(42, (B, T, dirs * H), 0.25))
