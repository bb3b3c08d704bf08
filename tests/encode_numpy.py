"""
TEST INFRASTRUCTURE ONLY: the three spike encoders restated in float32 numpy from the documented contract
(include/sparch_hip.h, "Spike encoders").  Shares no code with the product.

    z = (x - lo[k]) * scale[k]                      two fp32 roundings
    RATE : p = z > 0 ? min(z, 1) : 0 (NaN: 0); spike iff u < p, u = dropout_numpy.uniforms(seed) at the time-major
           index ((t0 + t) * B + b) * K + k
    IF   : drive = z > 0 ? min(z, 255) : 0; v += drive; n = floor(v); v -= n
    DELTA: fresh: local step 0 sets ref = z (0 if not finite), emits nothing; else e = z - ref,
           n = min(floor(|e|), 255), ON (column k) if e > 0, OFF (column K + k) if e < 0, ref += copysign(n, e);
           a z that is not finite emits nothing and leaves ref
    lengths: a step t >= lengths[b] emits 0 and leaves the state

Every function returns (counts (B,T,K') uint8, state (B,K) float32 or None); `outputs` derives the other forms.
"""
import numpy as np

from tests import dropout_numpy

F = np.float32
RATE, IF, DELTA = 0, 1, 2


def width(code, K):
    return 2 * K if code == DELTA else K


def _z(x, lo, scale):
    x, lo, scale = np.asarray(x, F), np.asarray(lo, F), np.asarray(scale, F)
    with np.errstate(all="ignore"):
        return ((x - lo[None, None, :]).astype(F) * scale[None, None, :]).astype(F)


def _valid(B, T, lengths):
    if lengths is None:
        return np.ones((B, T), bool)
    return np.arange(T)[None, :] < np.asarray(lengths)[:, None]


def rate(x, lo, scale, seed, t0=0, lengths=None):
    B, T, K = x.shape
    z = _z(x, lo, scale)
    with np.errstate(invalid="ignore"):
        p = np.where(z > 0, np.minimum(z, F(1)), F(0)).astype(F)
    u = dropout_numpy.uniforms(seed, T * B * K, first_index=t0 * B * K).reshape(T, B, K).transpose(1, 0, 2)
    n = (u < p) & _valid(B, T, lengths)[:, :, None]
    return n.astype(np.uint8), None


def integrate_fire(x, lo, scale, state=None, lengths=None):
    """state None = fresh (v starts at 0)."""
    B, T, K = x.shape
    z = _z(x, lo, scale)
    with np.errstate(invalid="ignore"):
        drive = np.where(z > 0, np.minimum(z, F(255)), F(0)).astype(F)
    v = np.zeros((B, K), F) if state is None else np.array(state, F)
    ok = _valid(B, T, lengths)
    out = np.zeros((B, T, K), np.uint8)
    for t in range(T):
        s = (v + drive[:, t]).astype(F)
        n = np.floor(s).astype(F)
        live = ok[:, t][:, None]
        out[:, t] = np.where(live, n, 0).astype(np.uint8)
        v = np.where(live, (s - n).astype(F), v)
    return out, v


def delta(x, lo, scale, state=None, lengths=None):
    """state None = fresh (ref starts at 0, local step 0 sets it and emits nothing)."""
    B, T, K = x.shape
    z = _z(x, lo, scale)
    fresh = state is None
    ref = np.zeros((B, K), F) if fresh else np.array(state, F)
    ok = _valid(B, T, lengths)
    out = np.zeros((B, T, 2 * K), np.uint8)
    with np.errstate(all="ignore"):
        for t in range(T):
            zt = z[:, t]
            fin = np.isfinite(zt)
            live = ok[:, t][:, None]
            if fresh and t == 0:
                ref = np.where(live, np.where(fin, zt, F(0)), ref).astype(F)
                continue
            e = (zt - ref).astype(F)
            n = np.where(fin & ~np.isnan(e), np.minimum(np.floor(np.abs(e)), F(255)), F(0)).astype(F)
            moved = (ref + np.copysign(n, e)).astype(F)
            emit = np.where(live, n, 0).astype(np.uint8)
            out[:, t, :K] = np.where(e > 0, emit, 0)
            out[:, t, K:] = np.where(e < 0, emit, 0)
            ref = np.where(live & fin, moved, ref)
    return out, ref


def encode(code, x, lo, scale, state=None, lengths=None, seed=0, t0=0):
    if code == RATE:
        return rate(x, lo, scale, seed, t0, lengths)
    if code == IF:
        return integrate_fire(x, lo, scale, state, lengths)
    return delta(x, lo, scale, state, lengths)


def chunked(code, x, lo, scale, splits, seed=0):
    """The sequence cut at `splits` (chunk lengths; the rest is the last chunk), state and t0 carried."""
    T = x.shape[1]
    cuts, at = [], 0
    for n in splits:
        if at + n > T:
            break
        cuts.append((at, at + n))
        at += n
    if at < T:
        cuts.append((at, T))
    state, parts = None, []
    for a, b in cuts:
        c, state = encode(code, x[:, a:b], lo, scale, state=state, seed=seed, t0=a)
        parts.append(c)
    return np.concatenate(parts, axis=1), state


def outputs(counts, ldp=None):
    """(dense fp32, plane (B*T, ldp) uint16 bf16 bit patterns with zero pad columns, totals (K') uint32)."""
    B, T, KW = counts.shape
    ldp = (KW + 7) // 8 * 8 if ldp is None else ldp
    dense = counts.astype(F)
    plane = np.zeros((B * T, ldp), np.uint16)
    plane[:, :KW] = (dense.reshape(B * T, KW).view(np.uint32) >> 16).astype(np.uint16)
    totals = counts.reshape(B * T, KW).astype(np.uint64).sum(0).astype(np.uint32)
    return dense, plane, totals
