"""
The selectable readout (sparch_readout_fwd_red / sparch_readout_bwd_red, SNN(readout=...)) restated on the host, beside
tests/spiking_numpy.py readout_forward / readout_backward, whose recurrence, softmax and parameter sums it imports.

    forward(dtype, Wx, scale, shift, alpha, u0, mode, lengths=None, class_order=None) -> dict(u_save, out[, arg])
        T_b = lengths[b] (T without lengths).  out[b, c] per mode:
          softmax_sum   sum_{t < T_b} softmax(u_t)[c], one sequential sum in `dtype` in time order (without lengths:
                        spiking_numpy.readout_forward's own arrays)
          softmax_mean  that accumulator / dtype(T_b)
          u_max         max_{t < T_b} u_t[c], and arg (B,C) the EARLIEST step that reaches it (u0 is no candidate)
          u_mean        ((u_0 + u_1) + u_2 ...) / dtype(T_b), one chain in `dtype` in time order
          u_last        u_{T_b - 1}[c]
    backward(dtype, g_out, mode, u_save, alpha, u0, bn=None, lengths=None, arg=None, class_order=None)
        -> dict(dWx, ws_alpha, alpha[, bn_dy, bn_dyx]) on supplied saves: the direct gradient e_t into u_t, then
        spiking_numpy.readout_backward's reverse recurrence (softmax_sum without lengths: that function itself).
          softmax_sum   p_t (g - <p_t, g>)         softmax_mean  the same with g / dtype(T_b) for g
          u_max         g[c] at t = arg[b, c], else 0 (arg None: taken from u_save)
          u_mean        g[c] / dtype(T_b) at every t < T_b        u_last  g[c] at t = T_b - 1, else 0
        Nothing is looked at for t >= lengths[b] (a NaN there changes nothing) and dWx is 0 there.
    torch_forward(Wx, alpha, u0, mode, lengths=None) -> out: the same formulas in torch, what autograd differentiates.
"""
import numpy as np
import torch

from tests import spiking_numpy as sn
from tests.kit import F32

MODES = ("softmax_sum", "softmax_mean", "u_max", "u_mean", "u_last")
MEAN_MODES = ("softmax_mean", "u_mean")


def valid(lengths, B, T):
    """(B, T) bool: t < lengths[b] (all true without lengths)."""
    if lengths is None:
        return np.ones((B, T), bool)
    return np.arange(T)[None, :] < np.asarray(lengths)[:, None]


def steps_of(lengths, B, T):
    """(B,) integers: T_b."""
    return np.full(B, T, np.int64) if lengths is None else np.asarray(lengths, np.int64)


def first_argmax(u_save, lengths=None):
    """(B,C) int32: the earliest step of each class's maximum over the row's own steps."""
    U = np.asarray(u_save)
    m = valid(lengths, U.shape[0], U.shape[1])[:, :, None]
    return np.where(m, U, -np.inf).argmax(1).astype(np.int32)


def _time_sum(q, dtype):
    """One sequential sum over axis 1 in `dtype`, ascending."""
    return sn.ordered_sum(q.astype(dtype), 1, "asc")


def forward(dtype, Wx, scale, shift, alpha, u0, mode, lengths=None, class_order=None):
    assert mode in MODES, mode
    U, out_sum = sn.readout_forward(dtype, Wx, scale, shift, alpha, u0, class_order)
    if mode == "softmax_sum" and lengths is None:
        return {"u_save": U, "out": out_sum}
    B, T, C = U.shape
    m = valid(lengths, B, T)[:, :, None]
    n = steps_of(lengths, B, T).astype(dtype)[:, None]
    res = {"u_save": U}
    if mode in ("softmax_sum", "softmax_mean"):
        acc = _time_sum(np.where(m, sn._softmax(U, class_order), dtype(0)), dtype)
        res["out"] = acc if mode == "softmax_sum" else (acc / n).astype(dtype)
    elif mode == "u_max":
        res["arg"] = first_argmax(U, lengths)
        res["out"] = np.take_along_axis(U, res["arg"][:, None, :].astype(np.int64), 1)[:, 0]
    elif mode == "u_mean":
        res["out"] = (_time_sum(np.where(m, U, dtype(0)), dtype) / n).astype(dtype)
    else:
        res["out"] = U[np.arange(B), steps_of(lengths, B, T) - 1]
    return res


def backward(dtype, g_out, mode, u_save, alpha, u0, bn=None, lengths=None, arg=None, class_order=None):
    assert mode in MODES, mode
    if mode == "softmax_sum" and lengths is None:
        return sn.readout_backward(dtype, g_out, u_save, alpha, u0, bn=bn, class_order=class_order)
    B, T, C = np.asarray(u_save).shape
    m = valid(lengths, B, T)[:, :, None]
    steps = steps_of(lengths, B, T)
    U = np.where(m, np.asarray(u_save), 0).astype(dtype)
    g = np.asarray(g_out, dtype=dtype)
    if mode in MEAN_MODES:
        g = (g / steps.astype(dtype)[:, None]).astype(dtype)
    t_of = np.arange(T)[None, :, None]
    if mode in ("softmax_sum", "softmax_mean"):
        p = sn._softmax(U, class_order)
        dot = sn.ordered_sum(p * g[:, None, :], -1, class_order)
        e = p * (g[:, None, :] - dot[..., None])
    elif mode == "u_max":
        a = first_argmax(u_save, lengths) if arg is None else np.asarray(arg)
        e = np.where(t_of == a[:, None, :], g[:, None, :], dtype(0))
    elif mode == "u_mean":
        e = np.broadcast_to(g[:, None, :], (B, T, C))
    else:
        e = np.where(t_of == (steps - 1)[:, None, None], g[:, None, :], dtype(0))
    e = np.where(m, e, dtype(0)).astype(dtype)
    raw = np.asarray(alpha, dtype=F32)
    lo, hi = sn.LIMS["alpha"]
    al = np.minimum(np.maximum(raw.astype(dtype), dtype(lo)), dtype(hi))
    oma = dtype(1) - al
    du, acc = np.zeros((B, C), dtype), np.zeros((B, C), dtype)
    dWx = np.empty((B, T, C), dtype)
    for t in range(T - 1, -1, -1):          # (tests/spiking_numpy.py readout_backward's loop)
        du = al * du + e[:, t]
        dWx[:, t] = oma * du
        acc = acc + du * ((U[:, t - 1] if t > 0 else np.asarray(u0, dtype=dtype)) - U[:, t])
    ws = acc / oma
    out = {"dWx": dWx, "ws_alpha": ws,
           "alpha": np.where(sn.inside(raw, sn.LIMS["alpha"]), sn.ordered_sum(ws, 0, class_order), dtype(0))}
    if bn is not None:
        x_raw, mean, invstd = (np.asarray(v, dtype=dtype) for v in bn)
        xhat = np.where(m, (x_raw - mean) * invstd, dtype(0))
        rows = lambda q: q if class_order is None else sn.ordered_sum(q[:, ::-1], 1, "asc")  # noqa: E731
        tot = (lambda q: q.sum((0, 1))) if class_order is None else (lambda q: sn.ordered_sum(rows(q), 0, class_order))
        out["bn_dy"], out["bn_dyx"] = tot(dWx), tot(dWx * xhat)
    return out


def torch_forward(Wx, alpha, u0, mode, lengths=None):
    """out (B,C) in Wx's dtype, differentiable."""
    assert mode in MODES, mode
    B, T, C = Wx.shape
    lo, hi = (float(v) for v in sn.LIMS["alpha"])
    al = torch.clamp(alpha, min=lo, max=hi)
    u, us = u0, []
    for t in range(T):
        u = al * u + (1 - al) * Wx[:, t, :]
        us.append(u)
    steps = steps_of(lengths, B, T)
    rows = []
    for b in range(B):
        Ub = torch.stack([q[b] for q in us[:int(steps[b])]], 0)     # the row's own steps (T_b, C)
        if mode == "softmax_sum":
            rows.append(torch.softmax(Ub, 1).sum(0))
        elif mode == "softmax_mean":
            rows.append(torch.softmax(Ub, 1).sum(0) / int(steps[b]))
        elif mode == "u_max":
            rows.append(Ub.max(0).values)
        elif mode == "u_mean":
            rows.append(Ub.sum(0) / int(steps[b]))
        else:
            rows.append(Ub[-1])
    return torch.stack(rows, 0)
