"""
The host restatement of the synaptic currents (tests/synapse_numpy.py) and the network cases' oracle
(tests/synapse_cases.py), checked against themselves — no GPU.

  * the fp64 backward equals central differences of the fp64 forward (g_z, g_gamma), with lengths and a carried i0;
  * g_gamma from the saved i, (i[t-1] - i[t]) / (1 - g), equals its definition through i[t-1] - z[t];
  * the acceptance bound of g_gamma (derived in tests/synapse_numpy.py) sees a lost term: dropping the t = 0 terms, one
    batch row or the gate leaves it; the fp32 restatement of the kernel's arithmetic stays inside it with a factor of
    at least 4 to spare;
  * fma32 is a fused multiply-add;
  * every network case of tests/synapse_cases.py is kept by the rule of tests/network_cases.py at its committed data
    seed (MARGIN = 8, every hidden layer's rate inside RATE_WINDOW), and that seed is the first that keeps it: no case
    is left out.

The first four groups exercise tests/synapse_numpy.py alone — the reference the device is held to has to be right before
anything is compared with it — and so do not depend on the package: they pass with or without the feature.  The network
cases build SNN(synapse=...) and fail without it, as every test of tests/test_synapse_host.py and
tests/test_synapse_gpu.py does.
"""
from fractions import Fraction

import numpy as np
import pytest

from tests import synapse_cases as sc
from tests import synapse_numpy as syn
from tests.kit import F32, F64

SHAPES = [(H, lim, lengths) for H in sc.WIDTHS for lim in sc.LIMITS for lengths in (None, sc.LENGTHS)]


def data(H, lim):
    d = sc.kernel_data(H)
    gamma = sc.gammas(H, *lim)
    z = syn.drive(d["Wx"], d["bias"], d["scale"], d["shift"], F64)
    return d, gamma, z


def test_fma32_rounds_once():
    rng = np.random.default_rng(5)
    x, a, b = (rng.standard_normal(4000).astype(F32) for _ in range(3))
    b[:2000] = -(x[:2000].astype(F64) * a[:2000]).astype(F32)          # cancellation: where two roundings differ
    got = syn.fma32(x, a, b)
    twice = (x * a + b).astype(F32)
    for k in range(x.size):
        exact = Fraction(float(x[k])) * Fraction(float(a[k])) + Fraction(float(b[k]))
        lo_, hi_ = sorted((np.nextafter(got[k], F32(-np.inf)), np.nextafter(got[k], F32(np.inf))))
        assert abs(exact - Fraction(float(got[k]))) <= min(abs(exact - Fraction(float(lo_))), abs(exact - Fraction(float(hi_))))
    assert (got != twice).any()


@pytest.mark.parametrize("H,lim,lengths", SHAPES)
def test_backward_is_the_derivative_of_the_forward(H, lim, lengths):
    d, gamma, z = data(H, lim)
    # inside the limits, off their edges: the clamp is differentiable there (the gate is tested below)
    gamma = np.clip(gamma, lim[0] + 0.01, lim[1] - 0.01).astype(F32)
    g = d["g"].astype(F64)
    valid = np.arange(sc.T)[None, :, None] < np.asarray(lengths or [sc.T] * sc.B)[:, None, None]

    def loss(zz, gm):
        i, _ = syn.forward(zz, gm, *lim, d["i0"], lengths, F64)
        return float((i * g * valid).sum())

    i, _ = syn.forward(z, gamma, *lim, d["i0"], lengths, F64)
    g_z = syn.backward_z(g, gamma, *lim, lengths, F64)
    g_gamma, _ = syn.backward_gamma(g, i, gamma, *lim, d["i0"], lengths)
    eps = 1e-6
    rng = np.random.default_rng(1)
    for _ in range(6):
        b, t, h = rng.integers(sc.B), rng.integers(sc.T), rng.integers(H)
        dz = np.zeros_like(z)
        dz[b, t, h] = eps
        fd = (loss(z + dz, gamma.astype(F64)) - loss(z - dz, gamma.astype(F64))) / (2 * eps)
        assert abs(fd - g_z[b, t, h]) <= 1e-7 * max(1.0, abs(fd)), (b, t, h)
    for h in range(H):
        dg = np.zeros(H)
        dg[h] = eps
        fd = (loss_raw(z, gamma.astype(F64) + dg, d, lengths, g, valid) - loss_raw(z, gamma.astype(F64) - dg, d, lengths, g, valid)) / (2 * eps)
        assert abs(fd - g_gamma[h]) <= 1e-6 * max(1.0, abs(fd)), h


def loss_raw(z, gamma64, d, lengths, g, valid):
    """The forward with an fp64 gamma (syn.forward takes the fp32 parameter)."""
    B, T, H = z.shape
    st = d["i0"].astype(F64).copy()
    total = 0.0
    for b, n in enumerate(lengths or [T] * B):
        for t in range(n):
            st[b] = gamma64 * st[b] + (1.0 - gamma64) * z[b, t]
            total += float((st[b] * g[b, t]).sum())
    return total


@pytest.mark.parametrize("H,lim,lengths", SHAPES)
def test_the_saved_current_gives_the_gradient_of_gamma(H, lim, lengths):
    d, gamma, z = data(H, lim)
    i, _ = syn.forward(z, gamma, *lim, d["i0"], lengths, F64)
    from_i, mag = syn.backward_gamma(d["g"], i, gamma, *lim, d["i0"], lengths)
    direct = syn.backward_gamma_direct(d["g"], z, gamma, *lim, d["i0"], lengths)
    assert (mag > 0).all() and (from_i != 0).any()
    assert np.abs(from_i - direct).max() <= 1e-12 * np.abs(direct).max()
    gate = syn.gate(gamma, *lim)
    assert (gate == 0).any() and (gate == 1).any() and not from_i[gate == 0].any()


@pytest.mark.parametrize("H,lim,lengths", SHAPES)
def test_the_bound_sees_a_lost_term_and_holds_the_fp32_restatement(H, lim, lengths):
    d, gamma, z = data(H, lim)
    i, _ = syn.forward(z, gamma, *lim, d["i0"], lengths, F64)
    ref, _ = syn.backward_gamma(d["g"], i, gamma, *lim, d["i0"], lengths)
    bound = syn.gamma_bound(d["g"], z, gamma, *lim, d["i0"], lengths)
    open_ = syn.gate(gamma, *lim) == 1
    # (tight enough to mean something: under 1e-3 of the gradient even at g = 0.9, where 1 / oma and the carried errors
    # of two scans of up to T steps each multiply the unit roundoff by a few thousand)
    assert (bound > 0).all() and (bound[open_] <= 1e-3 * np.maximum(np.abs(ref[open_]), 1.0)).all()
    for kw in (dict(skip_first=True), dict(skip_row=0), dict(gated=False)):
        wrong, _ = syn.backward_gamma(d["g"], i, gamma, *lim, d["i0"], lengths, **kw)
        assert (np.abs(wrong - ref) > bound).any(), kw
    # the kernel's arithmetic, restated: fp32 forward, fp32 adjoint, the products summed in fp32 row after row
    z32 = syn.drive(d["Wx"], d["bias"], d["scale"], d["shift"], F32)
    i32, _ = syn.forward(z32, gamma, *lim, d["i0"], lengths, F32)
    a32 = syn.adjoint(d["g"], gamma, *lim, lengths, F32)
    prev = np.concatenate([d["i0"][:, None], i32[:, :-1]], axis=1)
    acc = np.zeros(H, F32)
    for b, n in enumerate(lengths or [sc.T] * sc.B):
        for t in range(n):
            acc = acc + a32[b, t] * (prev[b, t] - i32[b, t])
    got = acc / (F32(1.0) - syn.clamped(gamma, *lim)) * syn.gate(gamma, *lim).astype(F32)
    assert got.dtype == F32
    assert (np.abs(got.astype(F64) - ref) * 4 <= bound).all()


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_every_network_case_is_kept_at_its_committed_seed(c):
    seed = sc.SEEDS[c]
    kept, why = sc.verdict(c, seed)
    assert kept, why
    assert sc.pick_seed(c, seed + 1) == seed                # the first seed that keeps it
    _, _, r64, _ = sc.runs(c, seed)
    gm = {k: v for k, v in r64["grads"].items() if k.endswith("gamma")}
    assert len(gm) == 2 and all(bool(v.any()) and float(v[0]) == 0.0 for v in gm.values())   # column 0: clamped
