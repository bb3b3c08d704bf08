"""
CPU: tests/encode_numpy.py, the restatement the GPU tests compare the spike encoders with, pinned on dyadic inputs
(multiples of 1/64 of moderate size: every fp32 sum and difference below is exact), where the codes' invariants hold
as equalities.
"""
import os
import re

import numpy as np
import pytest

from tests import encode_numpy as en

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def contract():
    """What is restated is the header's contract: its section exists and numbers the codes as the restatement does."""
    with open(os.path.join(ROOT, "include", "sparch_hip.h")) as f:
        header = f.read()
    assert "int sparch_spike_encode(" in header and "---- Spike encoders" in header
    for name, code in (("RATE", en.RATE), ("IF", en.IF), ("DELTA", en.DELTA)):
        assert re.search(rf"#define SPARCH_ENCODE_{name} {code}\b", header), name


def dyadic(shape, seed, lo=-2.0, hi=6.0):
    rng = np.random.default_rng(seed)
    return (rng.integers(int(lo * 64), int(hi * 64), size=shape) / 64.0).astype(F)


ONE = lambda K: (np.zeros(K, F), np.ones(K, F))  # noqa: E731  (lo = 0, scale = 1: z = x)


def test_if_conserves_the_drive_exactly():
    B, T, K = 3, 40, 5
    x = dyadic((B, T, K), 1)
    lo, scale = np.full(K, -0.5, F), np.full(K, 0.25, F)          # dyadic too: z is exact
    n, v = en.integrate_fire(x, lo, scale)
    z = (x - lo) * scale
    drive = np.where(z > 0, np.minimum(z, 255), 0).astype(np.float64)
    assert n.dtype == np.uint8 and n.any() and (v >= 0).all() and (v < 1).all()
    assert np.array_equal(n.sum(1).astype(np.float64) + v.astype(np.float64), drive.sum(1))


def test_if_clamps_the_drive_at_255():
    x = np.array([[[1000.0], [np.inf], [0.5], [0.5]]], F)
    n, v = en.integrate_fire(x, *ONE(1))
    assert n[0, :, 0].tolist() == [255, 255, 0, 1] and v[0, 0] == 0


def test_delta_tracks_within_one_threshold():
    B, T, K = 2, 50, 4
    x = dyadic((B, T, K), 2, -3.0, 3.0)
    lo, scale = ONE(K)
    ref = None
    for t in range(T):                                            # one step at a time: the state after every step
        c, ref = en.delta(x[:, t:t + 1], lo, scale, state=ref)
        assert (c < 255).all()
        assert (np.abs(x[:, t] - ref) < 1).all(), t
        assert not (c[:, 0, :K].astype(bool) & c[:, 0, K:].astype(bool)).any()      # ON and OFF never both
    whole, ref_w = en.delta(x, lo, scale)
    assert np.array_equal(ref_w, ref) and whole.any()
    # the reference moved by what was sent
    net = whole[:, :, :K].astype(np.int64).sum(1) - whole[:, :, K:].astype(np.int64).sum(1)
    assert np.array_equal(x[:, 0] + net, ref_w)


def test_delta_saturates_a_jump_of_300():
    x = np.array([[[0.0], [300.0], [300.0], [300.0], [-10.0]]], F)
    c, ref = en.delta(x, *ONE(1))
    assert c[0, :, 0].tolist() == [0, 255, 45, 0, 0] and c[0, :, 1].tolist() == [0, 0, 0, 0, 255]
    assert ref[0, 0] == 45.0


@pytest.mark.parametrize("code", [en.RATE, en.IF, en.DELTA])
@pytest.mark.parametrize("splits", [[1, 3], [5], [1, 1, 1, 1], [16]])
def test_chunked_equals_whole(code, splits):
    B, T, K = 3, 17, 5
    x = dyadic((B, T, K), 3, -1.0, 3.0)
    lo, scale = np.full(K, -0.25, F), np.full(K, 0.5, F)
    whole, state = en.encode(code, x, lo, scale, seed=77)
    parts, state_c = en.chunked(code, x, lo, scale, splits, seed=77)
    assert whole.shape == (B, T, en.width(code, K)) and whole.any()
    assert np.array_equal(whole, parts)
    assert state is None and state_c is None if code == en.RATE else np.array_equal(state.view(np.uint32), state_c.view(np.uint32))


@pytest.mark.parametrize("code", [en.IF, en.DELTA])
def test_non_finite_rows_emit_nothing_and_keep_the_state(code):
    K = 3
    x = dyadic((1, 6, K), 4, 0.0, 4.0)
    bad = x.copy()
    bad[0, 2] = [np.nan, np.inf, -np.inf]
    bad[0, 4] = np.nan
    lo, scale = ONE(K)
    before, s_before = en.encode(code, bad[:, :2], lo, scale)
    c, s = en.encode(code, bad[:, 2:3], lo, scale, state=s_before)
    if code == en.IF:          # +inf drives at the clamp: 255 spikes and the fraction stays; NaN and -inf give nothing
        assert c[0, 0].tolist() == [0, 255, 0]
    else:
        assert not c.any()
    assert np.array_equal(s.view(np.uint32), s_before.view(np.uint32))
    whole, _ = en.encode(code, bad, lo, scale)
    assert not whole[0, 4].any()
    if code == en.DELTA:       # a fresh stream whose first value is not finite starts its reference at 0
        c0, r0 = en.delta(np.array([[[np.nan], [2.5]]], F), *ONE(1))
        assert c0[0, :, 0].tolist() == [0, 2] and r0[0, 0] == 2.0


def test_lengths_stop_the_emission_and_the_state():
    B, T, K = 4, 9, 3
    x = dyadic((B, T, K), 5, 0.0, 3.0)
    lo, scale = np.zeros(K, F), np.full(K, 0.75, F)
    lengths = [1, 2, T - 1, T]
    for code in (en.RATE, en.IF, en.DELTA):
        c, s = en.encode(code, x, lo, scale, lengths=lengths, seed=5)
        assert c.any()
        for b, n in enumerate(lengths):
            assert not c[b, n:].any()
            cb, sb = en.encode(code, x[b:b + 1, :n], lo, scale, seed=5)
            if code != en.RATE:                                    # (a row's draws depend on B: not comparable alone)
                assert np.array_equal(c[b, :n], cb[0]) and np.array_equal(s[b], sb[0])


def test_rate_mean_is_p_and_the_index_is_time_major():
    K = 1 << 16
    x = np.full((1, 1, K), 0.3, F)
    c, _ = en.rate(x, *ONE(K), seed=123)
    mean, sigma = c.mean(), np.sqrt(0.3 * 0.7 / K)
    assert abs(mean - 0.3) < 4 * sigma
    # p = 0 and p = 1; a NaN gives 0
    edge = np.array([[[-1.0, 0.0, 1.0, 7.0, np.nan]]], F)
    assert en.rate(edge, *ONE(5), seed=9)[0][0, 0].tolist() == [0, 0, 1, 1, 0]
    # element (b, t, k) draws index ((t0 + t) * B + b) * K + k
    from tests import dropout_numpy
    B, T, Kk, t0 = 2, 3, 4, 5
    xs = np.full((B, T, Kk), 0.5, F)
    got, _ = en.rate(xs, *ONE(Kk), seed=11, t0=t0)
    for b in range(B):
        for t in range(T):
            u = dropout_numpy.uniforms(11, Kk, first_index=((t0 + t) * B + b) * Kk)
            assert got[b, t].tolist() == (u < F(0.5)).astype(int).tolist()


def test_outputs_plane_is_bf16_of_the_counts_with_zero_pad():
    c = np.array([[[0, 1, 2, 255, 128]]], np.uint8)
    dense, plane, totals = en.outputs(c)
    assert plane.shape == (1, 8) and plane[0, 5:].tolist() == [0, 0, 0]
    assert plane[0, :5].tolist() == [0, 0x3F80, 0x4000, 0x437F, 0x4300]
    assert dense.dtype == F and totals.tolist() == [0, 1, 2, 255, 128]
    assert en.outputs(c, ldp=16)[1].shape == (1, 16)
