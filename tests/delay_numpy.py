"""
Axonal delays restated in numpy, fp64 ("Axonal delays"; include/sparch_hip.h, sparch_delay_*).

With d_i = rint(clamp(theta_i, 0, D)) (ties to even), len_b the row's own length (T without lengths) and x[b,-1,i] = 0:

    y[b,t,i]   = x[b, t - d_i, i]      if d_i <= t < len_b,  else 0
    g_x[b,t,i] = g_y[b, t + d_i, i]    if t + d_i < len_b,   else 0
    g_th[i]    = gate_i * sum_b sum_{t = d_i}^{len_b - 1} g_y[b,t,i] * (x[b,t-d_i-1,i] - x[b,t-d_i,i])
    gate_i     = 1 if 0 <= theta_i <= D else 0

Plain loops over (b, i): the restatement is meant to be read, the shapes it runs on are tiny.
"""
import numpy as np

F64 = np.float64


def steps(theta, D):
    """The integer delays the kernels take, (K,) int64."""
    theta = np.asarray(theta, np.float32)
    return np.rint(np.clip(np.where(np.isnan(theta), 0.0, theta), 0.0, float(D))).astype(np.int64)


def gate(theta, D):
    theta = np.asarray(theta, np.float32)
    return ((theta >= 0) & (theta <= D)).astype(F64)


def _lengths(lengths, B, T):
    return np.full(B, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)


def forward(x, theta, D, lengths=None):
    """y (B,T,K) in x's dtype: a copy of x's elements, or zeros."""
    x = np.asarray(x)
    B, T, K = x.shape
    d, lens = steps(theta, D), _lengths(lengths, B, T)
    y = np.zeros_like(x)
    for b in range(B):
        for i in range(K):
            n = int(lens[b]) - int(d[i])
            if n > 0:
                y[b, d[i]:lens[b], i] = x[b, :n, i]
    return y


def backward_x(g_y, theta, D, lengths=None):
    """g_x (B,T,K) in g_y's dtype; what g_y holds at t >= len_b is never read."""
    g_y = np.asarray(g_y)
    B, T, K = g_y.shape
    d, lens = steps(theta, D), _lengths(lengths, B, T)
    g_x = np.zeros_like(g_y)
    for b in range(B):
        for i in range(K):
            n = int(lens[b]) - int(d[i])
            if n > 0:
                g_x[b, :n, i] = g_y[b, d[i]:lens[b], i]
    return g_x


def backward_theta(g_y, x, theta, D, lengths=None):
    """(g_theta (K,) fp64, the sum of |g_y * dx| per column (K,) fp64 — what the error bound of an fp32 sum scales
    with)."""
    g_y, x = np.asarray(g_y, F64), np.asarray(x, F64)
    B, T, K = x.shape
    d, lens = steps(theta, D), _lengths(lengths, B, T)
    g, mag = np.zeros(K, F64), np.zeros(K, F64)
    for b in range(B):
        for i in range(K):
            for t in range(int(d[i]), int(lens[b])):
                s = t - int(d[i])
                dx = (x[b, s - 1, i] if s >= 1 else 0.0) - x[b, s, i]
                g[i] += g_y[b, t, i] * dx
                mag[i] += abs(g_y[b, t, i] * dx)
    return g * gate(theta, D), mag


def stream(chunks, theta, D):
    """The chunks (B,Tc,K) of a stream delayed one by one with a carried history (B,D,K) of the last D input steps
    (zeros at the start) -> the list of delayed chunks; their concatenation is forward() of the concatenated input."""
    chunks = [np.asarray(c) for c in chunks]
    B, _, K = chunks[0].shape
    d = steps(theta, D)
    hist = np.zeros((B, D, K), chunks[0].dtype)
    out = []
    for c in chunks:
        both = np.concatenate([hist, c], axis=1)
        y = np.empty_like(c)
        for i in range(K):
            y[:, :, i] = both[:, D - d[i]:D - d[i] + c.shape[1], i]
        out.append(y)
        hist = both[:, -D:]
    return out
