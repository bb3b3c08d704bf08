"""
Plain numpy fp64 restatements of the G2 kernels of include/sparch_hip.h (sparch_amd/csrc/norm.hip): what each entry
point computes, written as the formula and nothing else — no tiling, no summation order, no fp32.  The GPU tests
(tests/test_norm_kernels_gpu.py) compare the kernels with these; tests/test_norm_numpy_host.py pins these against
torch fp64 (batch_norm, layer_norm, autograd, torch.clamp's backward) without a GPU.

Every function takes array-likes, computes in float64 and returns float64 arrays (the planes: uint16).
"""
import numpy as np

BN_MOMENTUM = 0.05   # nn.BatchNorm1d(H, momentum=0.05), snns.py:240
NORM_EPS = 1e-5


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---------------------------------------------------------------------------------------------- BatchNorm forward
def tile_partials(x, tile=128):
    """Per-row-tile column sums and sums of squares of x (M, H): two (ceil(M/tile), H) arrays, the layout the GEMM
    epilogue hands sparch_bn_finalize."""
    x = _f64(x)
    M = x.shape[0]
    cuts = range(0, M, tile)
    return (np.stack([x[r:r + tile].sum(0) for r in cuts]), np.stack([(x[r:r + tile] ** 2).sum(0) for r in cuts]))


def bn_finalize(s, ss, M, dup, gamma, beta, running_mean, running_var, momentum=BN_MOMENTUM, eps=NORM_EPS):
    """Training-mode finalize from partials s, ss (n_tiles, H) of M rows: batch mean, biased variance (clamped at 0),
    unbiased variance with n = dup * M, the running-statistics update, and the folded (scale, shift)."""
    S, SS = _f64(s).sum(0), _f64(ss).sum(0)
    mean = S / M
    var = np.maximum(SS / M - mean * mean, 0.0)
    n = float(dup) * float(M)
    unbiased = var * (n / (n - 1.0))
    invstd = 1.0 / np.sqrt(var + eps)
    scale = _f64(gamma) * invstd
    return dict(mean=mean, var=var, unbiased=unbiased, invstd=invstd, scale=scale,
                shift=_f64(beta) - mean * scale,
                running_mean=momentum * mean + (1.0 - momentum) * _f64(running_mean),
                running_var=momentum * unbiased + (1.0 - momentum) * _f64(running_var))


def bn_eval(gamma, beta, running_mean, running_var, eps=NORM_EPS):
    """Eval-mode fold: (scale, shift, invstd) from the running statistics."""
    invstd = 1.0 / np.sqrt(_f64(running_var) + eps)
    scale = _f64(gamma) * invstd
    return dict(mean=_f64(running_mean), invstd=invstd, scale=scale, shift=_f64(beta) - _f64(running_mean) * scale)


# ---------------------------------------------------------------------------------------------- BatchNorm backward
def bn_bwd_reduce(dy, x, mean, invstd):
    """(dgamma, dbeta) = (sum_m dy * xhat, sum_m dy), xhat = (x - mean) * invstd."""
    dy = _f64(dy)
    xhat = (_f64(x) - _f64(mean)) * _f64(invstd)
    return (dy * xhat).sum(0), dy.sum(0)


def bn_bwd_terms(dy, x, mean, invstd):
    """(sum_m |dy * xhat|, sum_m |dy|): what a rounding bound of bn_bwd_reduce is stated in."""
    dy = _f64(dy)
    xhat = (_f64(x) - _f64(mean)) * _f64(invstd)
    return np.abs(dy * xhat).sum(0), np.abs(dy).sum(0)


def bn_bwd_apply(dy, x, mean, invstd, gamma, dgamma, dbeta):
    """dx = gamma * invstd * (dy - dbeta / M - xhat * dgamma / M)."""
    dy = _f64(dy)
    M = dy.shape[0]
    xhat = (_f64(x) - _f64(mean)) * _f64(invstd)
    return _f64(gamma) * _f64(invstd) * (dy - _f64(dbeta) / M - xhat * _f64(dgamma) / M)


# ---------------------------------------------------------------------------------------------- LayerNorm
def layernorm_fwd(x, gamma, beta, Hn=None, eps=NORM_EPS):
    """y (M, H), mu (M), rstd (M): statistics over the leading Hn columns, y = 0 in columns Hn..H-1."""
    x = _f64(x)
    Hn = x.shape[1] if Hn is None else Hn
    xn = x[:, :Hn]
    mu = xn.mean(1)
    var = ((xn - mu[:, None]) ** 2).mean(1)
    rstd = 1.0 / np.sqrt(var + eps)
    y = np.zeros_like(x)
    y[:, :Hn] = (xn - mu[:, None]) * rstd[:, None] * _f64(gamma)[:Hn] + _f64(beta)[:Hn]
    return y, mu, rstd


def layernorm_bwd(dy, x, mu, rstd, gamma, Hn=None):
    """(dx, dgamma, dbeta) for given mu, rstd.  dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = gamma * dy,
    means over the leading Hn columns, dx = 0 behind them; dgamma = sum_m dy * xhat and dbeta = sum_m dy are taken
    over ALL H columns with xhat = (x - mu) * rstd (what the padding columns hold is finite and unused)."""
    dy, x = _f64(dy), _f64(x)
    Hn = x.shape[1] if Hn is None else Hn
    xhat = (x - _f64(mu)[:, None]) * _f64(rstd)[:, None]
    g = _f64(gamma)[:Hn] * dy[:, :Hn]
    s1 = g.mean(1, keepdims=True)
    s2 = (g * xhat[:, :Hn]).mean(1, keepdims=True)
    dx = np.zeros_like(x)
    dx[:, :Hn] = _f64(rstd)[:, None] * (g - s1 - xhat[:, :Hn] * s2)
    return dx, (dy * xhat).sum(0), dy.sum(0)


def layernorm_bwd_terms(dy, x, mu, rstd):
    dy = _f64(dy)
    xhat = (_f64(x) - _f64(mu)[:, None]) * _f64(rstd)[:, None]
    return np.abs(dy * xhat).sum(0), np.abs(dy).sum(0)


# ---------------------------------------------------------------------------------------------- column sums
def edge_values(lo, hi):
    """fp32 values around a clamp range: inside, the two ends, one ulp outside each, NaN."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    return np.array([0.5 * (lo32 + hi32), lo32, hi32, np.nextafter(lo32, np.float32(-np.inf)),
                     np.nextafter(hi32, np.float32(np.inf)), np.nan, np.nextafter(lo32, np.float32(np.inf)),
                     np.nextafter(hi32, np.float32(-np.inf))], dtype=np.float32)


def clamp_gate(raw, lo, hi):
    """1 where torch.clamp(raw, lo, hi) passes its gradient: lo <= raw <= hi, both ends included; 0 for NaN."""
    raw = _f64(raw)
    with np.errstate(invalid="ignore"):
        return ((raw >= lo) & (raw <= hi)).astype(np.float64)


def colsum_clamped(ws, raws=None, lims=None):
    """ws (n, rows, H) -> (n, H): out[j] = sum_r ws[j, r] where gate_j is open, +0 where it is closed.  raws: None or a list whose entries are None (no
    gate) or (H,) raw parameters; lims: None (nothing is gated) or (n, 2) [lo, hi]."""
    ws = _f64(ws)
    out = ws.sum(1)
    if raws is not None and lims is not None:
        for j, raw in enumerate(raws):
            if raw is not None:
                out[j] = np.where(clamp_gate(raw, float(lims[j][0]), float(lims[j][1])) != 0, out[j], 0.0)
    return out


# ---------------------------------------------------------------------------------------------- bf16 planes
def split3_planes(x):
    """The exact truncation split x = p0 + p1 + p2 of an fp32 array (M, H) as (3, M, H) uint16 bf16 bit patterns —
    tests/kit.split3_host (sparch_split3's restatement), not a second one."""
    import torch

    from tests.kit import split3_host
    x = np.ascontiguousarray(x, dtype=np.float32)
    p = split3_host(torch.from_numpy(x))                     # (3 * M, H) bf16
    return p.view(torch.int16).numpy().view(np.uint16).reshape((3,) + x.shape)


def planes_to_f32(planes):
    """(..., ) uint16 bf16 bit patterns -> the fp32 values they stand for."""
    return (np.asarray(planes, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)
