"""
Synaptic currents ("Synaptic currents"; csrc/synapse.hip) restated on the host, twice.

With g_h = clamp(gamma_h, lo, hi), z the cell's input (Wx (+ bias), then * scale + shift where a scale is given), len_b
the row's own length and i[b,-1,h] = i0[b,h]:

    i[b,t,h]   = g_h i[b,t-1,h] + (1 - g_h) z[b,t,h]                       0 <= t < len_b
    a[b,t,h]   = g_i[b,t,h] + g_h a[b,t+1,h],   a[b,len_b,h] = 0
    g_z[b,t,h] = (1 - g_h) a[b,t,h]
    g_gamma[h] = gate_h (sum_b sum_{t<len_b} a[b,t,h] (i[b,t-1,h] - i[b,t,h])) / (1 - g_h),   gate_h = [lo <= gamma_h <= hi]

dtype=F64: the formulas in fp64 on the fp32 parameters' values (the reference of every bound).  dtype=F32: the kernels'
expression tree — oma = 1.0f - g once per column, every step g*i + oma*z (two products, one add, each rounded), the
affine as a true fused multiply-add (fma32), a = g_i + g*a, g_z = oma*a — which the device has to match bit for bit.

gamma_bound() is the acceptance bound of g_gamma, from fp64 magnitudes alone (u = 2^-24):

  * the device adds B T products a (i[t-1] - i[t]) in fp32, in some order, and divides once by a rounded oma: at most
    (B T + 8) u sum |a dI| / oma, the 8 for the product, the difference, the quotient and oma (the g_theta bound of
    tests/test_delay_gpu.py, with its constant grown by the two extra operations);
  * its a and i are themselves fp32 scans.  A step of a = g_i + g a rounds twice, each by at most u times A_t, the same
    scan on |g_i|; the errors travel through the same recurrence, so |a32 - a64| <= 2 u AA_t with AA the scan of A.
    A step of i rounds three times on top of the affine's own rounding and the rounded oma: |i32 - i64| <= 5 u II_t with
    I the scan on |z| from |i0| and II the scan of I.  Into the sum they enter as |dI| 2 u AA_t + |a_t| 5 u (II_{t-1} +
    II_t), over oma.
"""
import numpy as np

from tests.kit import F32, F64

U = 2.0 ** -24
SUM_TERMS = 8


def fma32(x, a, b):
    """fl32(x a + b) with one rounding, for fp32 arrays: the product is exact in fp64, the sum is rounded to odd there
    (TwoSum gives its error), and an odd 53-bit value rounds to fp32 as the exact one does."""
    x, a, b = (np.asarray(v, F32).astype(F64) for v in (x, a, b))
    p = x * a
    s = p + b
    bb = s - p
    err = (p - (s - bb)) + (b - bb)
    s, err = np.broadcast_arrays(s, err)
    word = s.copy().view(np.int64)
    fix = (err != 0) & ((word & 1) == 0)
    away = (err > 0) == (s > 0)                       # the exact sum lies further from zero than s
    word = np.where(fix, np.where(away, word + 1, word - 1), word)
    return word.view(F64).astype(F32)


def clamped(gamma, lo, hi):
    """clamp(gamma, lo, hi) as the kernels take it: fp32 comparisons against the fp32 limits."""
    return np.minimum(np.maximum(np.asarray(gamma, F32), F32(lo)), F32(hi))


def gate(gamma, lo, hi):
    gamma = np.asarray(gamma, F32)
    return ((gamma >= F32(lo)) & (gamma <= F32(hi))).astype(F64)


def drive(Wx, bias=None, scale=None, shift=None, dtype=F64):
    """z: neuron_input of csrc/neuron.h."""
    if dtype == F32:
        z = np.asarray(Wx, F32)
        if bias is not None:
            z = z + np.asarray(bias, F32)
        if scale is not None:
            z = fma32(z, scale, np.zeros_like(np.asarray(scale, F32)) if shift is None else shift)
        return z
    z = np.asarray(Wx, F64)
    if bias is not None:
        z = z + np.asarray(bias, F64)
    if scale is not None:
        z = z * np.asarray(scale, F64) + (0.0 if shift is None else np.asarray(shift, F64))
    return z


def _lengths(lengths, B, T):
    return [T] * B if lengths is None else [int(v) for v in lengths]


def forward(z, gamma, lo, hi, i0=None, lengths=None, dtype=F64):
    """(i (B,T,H) with zeros on padded steps, i_T (B,H) the state after each row's last valid step)."""
    z = np.asarray(z, dtype)
    B, T, H = z.shape
    g = clamped(gamma, lo, hi).astype(dtype)
    oma = (F32(1.0) - clamped(gamma, lo, hi)).astype(dtype) if dtype == F32 else 1.0 - g
    st = np.zeros((B, H), dtype) if i0 is None else np.asarray(i0, dtype).copy()
    out = np.zeros((B, T, H), dtype)
    for b, n in enumerate(_lengths(lengths, B, T)):
        for t in range(n):
            st[b] = g * st[b] + oma * z[b, t]
            out[b, t] = st[b]
    return out, st


def adjoint(g_i, gamma, lo, hi, lengths=None, dtype=F64):
    """a (B,T,H), zeros on padded steps (g_i there is never read)."""
    g_i = np.asarray(g_i, dtype)
    B, T, H = g_i.shape
    g = clamped(gamma, lo, hi).astype(dtype)
    a = np.zeros((B, T, H), dtype)
    for b, n in enumerate(_lengths(lengths, B, T)):
        nxt = np.zeros(H, dtype)
        for t in range(n - 1, -1, -1):
            nxt = g_i[b, t] + g * nxt
            a[b, t] = nxt
    return a


def backward_z(g_i, gamma, lo, hi, lengths=None, dtype=F64):
    a = adjoint(g_i, gamma, lo, hi, lengths, dtype)
    c = clamped(gamma, lo, hi)
    oma = (F32(1.0) - c) if dtype == F32 else 1.0 - c.astype(F64)
    return oma.astype(dtype) * a


def _previous(i, i0):
    prev = np.empty_like(i)
    prev[:, 0] = 0.0 if i0 is None else np.asarray(i0, i.dtype)
    prev[:, 1:] = i[:, :-1]
    return prev


def backward_gamma(g_i, i, gamma, lo, hi, i0=None, lengths=None, skip_first=False, skip_row=None, gated=True):
    """(g_gamma (H,), mag (H,) = sum |a dI| / oma) in fp64 from the saved i.  skip_first / skip_row / gated=False: the
    same with the t = 0 terms, one batch row or the gate left out — what the bound has to see."""
    i = np.asarray(i, F64)
    B, T, H = i.shape
    a = adjoint(g_i, gamma, lo, hi, lengths, F64)
    oma = 1.0 - clamped(gamma, lo, hi).astype(F64)
    terms = a * (_previous(i, i0) - i)
    for b, n in enumerate(_lengths(lengths, B, T)):
        terms[b, n:] = 0.0
    mag = np.abs(terms).sum(axis=(0, 1)) / oma
    if skip_first:
        terms[:, 0] = 0.0
    if skip_row is not None:
        terms[skip_row] = 0.0
    total = terms.sum(axis=(0, 1)) / oma
    return (total * gate(gamma, lo, hi) if gated else total), mag


def backward_gamma_direct(g_i, z, gamma, lo, hi, i0=None, lengths=None):
    """g_gamma in fp64 from its definition, d i[t] / d g = i[t-1] - z[t]: sum a (i[t-1] - z[t])."""
    z = np.asarray(z, F64)
    B, T, H = z.shape
    i, _ = forward(z, gamma, lo, hi, i0, lengths, F64)
    a = adjoint(g_i, gamma, lo, hi, lengths, F64)
    terms = a * (_previous(i, i0) - z)
    for b, n in enumerate(_lengths(lengths, B, T)):
        terms[b, n:] = 0.0
    return terms.sum(axis=(0, 1)) * gate(gamma, lo, hi)


def _scan(x, g, start=None, reverse=False):
    """y[t] = x[t] + g y[t -+ 1] along axis 1 (y before the first step: start or 0)."""
    y = np.zeros_like(x)
    cur = np.zeros_like(x[:, 0]) if start is None else start.copy()
    steps = range(x.shape[1] - 1, -1, -1) if reverse else range(x.shape[1])
    for t in steps:
        cur = x[:, t] + g * cur
        y[:, t] = cur
    return y


def gamma_bound(g_i, z, gamma, lo, hi, i0=None, lengths=None):
    """The acceptance bound of g_gamma (H,), derived in the module docstring; everything in fp64."""
    z, g_i = np.asarray(z, F64), np.asarray(g_i, F64)
    B, T, H = z.shape
    L = _lengths(lengths, B, T)
    valid = np.arange(T)[None, :, None] < np.asarray(L)[:, None, None]
    g = clamped(gamma, lo, hi).astype(F64)
    oma = 1.0 - g
    i, _ = forward(z, gamma, lo, hi, i0, lengths, F64)
    a = adjoint(g_i, gamma, lo, hi, lengths, F64)
    start = np.zeros((B, H)) if i0 is None else np.abs(np.asarray(i0, F64))
    big_i = _scan(oma * np.abs(z) * valid, g, start)                    # I: the scan on |z| from |i0|
    big_ii = _scan(big_i * valid, g)                                    # II: the scan of I
    big_a = _scan(np.abs(np.where(valid, g_i, 0.0)), g, reverse=True)   # A, then AA
    big_aa = _scan(big_a * valid, g, reverse=True)
    d_i = np.abs(_previous(i, i0) - i) * valid
    ii_prev = np.zeros_like(big_ii)
    ii_prev[:, 1:] = big_ii[:, :-1]
    summed = (B * T + SUM_TERMS) * U * (np.abs(a) * d_i).sum(axis=(0, 1))
    carried = (d_i * 2 * U * big_aa + np.abs(a) * valid * 5 * U * (ii_prev + big_ii)).sum(axis=(0, 1))
    return (summed + carried) / oma


def bn_partials(g_z, x, mean, invstd, lengths=None):
    """BatchNorm backward's per-sequence partial sums as the backward scan adds them, in fp32 and in its order — from
    the row's last valid step to its first, acc_dy += g_z; acc_dyx += g_z * ((x - mean) * invstd), every operation
    rounded: ((B,H) sums of g_z, (B,H) sums of g_z xhat).  The device adds the B rows in double and rounds once."""
    g_z, x = np.asarray(g_z, F32), np.asarray(x, F32)
    mean, invstd = np.asarray(mean, F32), np.asarray(invstd, F32)
    B, T, H = g_z.shape
    dy, dyx = np.zeros((B, H), F32), np.zeros((B, H), F32)
    for b, n in enumerate(_lengths(lengths, B, T)):
        for t in range(n - 1, -1, -1):
            dy[b] = dy[b] + g_z[b, t]
            dyx[b] = dyx[b] + g_z[b, t] * ((x[b, t] - mean) * invstd)
    return dy, dyx
