"""
The per-step readout (sparch_readout_fwd_seq / sparch_readout_bwd_seq and their `_len` forms) restated on the host.

    forward(dtype, Wx, scale, shift, alpha, u0, mode, lengths=None, class_order=None)
        -> dict(u_save, out, seq): tests/spiking_numpy.py readout_forward's recurrence and softmax (imported), with
           seq (B,T,C) = softmax(u_t) ("prob") or the running sum of `out` after step t ("sum": ONE sequential sum in
           `dtype` in time order, whose last valid step is out itself); with lengths, seq is 0 and out stops at
           t >= lengths[b].
    backward(dtype, g_out, g_seq, mode, u_save, alpha, u0, bn=None, lengths=None, class_order=None)
        -> dict(dWx, ws_alpha, alpha[, bn_dy, bn_dyx]): the gradient of p_t is G_t = g_out + A_t, A_t = g_seq[t] ("prob") or
           the reverse running sum S_t = S_{t+1} + g_seq[t] ("sum", sequential in `dtype`); then e_t = p_t (G_t - <p_t, G_t>)
           and the reverse recurrence of tests/spiking_numpy.py readout_backward.  g_out None counts as 0; with lengths,
           g_seq and u_save are not looked at for t >= lengths[b] (a NaN there changes nothing) and dWx is 0 there.
    reverse_running_sum(g_seq, dtype=F32, lengths=None)   S as above, what the kernel's "thread = class" pass computes.
    torch_forward(Wx, alpha, u0, mode, lengths=None)      `_readout_cell` (oracle.snn_oracle.readout_cell's loop) with the
                                                          per-step output, in torch: what autograd differentiates.

Where the restatement comes from: the recurrence, the softmax with its ordered denominators and the parameter sums are
tests/spiking_numpy.py's (imported, the dtype-generic restatement that tests/test_readout_kernels_fp64_gpu.py holds the plain
kernels to); the oracle's own readout (oracle.bptt_numpy.readout_forward / readout_backward, fp32 only, one gradient row
per clip) cannot carry a per-step gradient or run in fp64, so it is the anchor instead: check_against_oracle() asserts
that with g_seq = 0 this file gives its dWx and dalpha, that the "sum" rows are its `out` on every prefix bit for bit,
and tests/test_readout_seq_host.py holds the fp64 runs to torch autograd.
"""
import numpy as np
import torch

from oracle import bptt_numpy as bptt
from tests import spiking_numpy as sn
from tests.kit import F32, F64

MODES = ("prob", "sum")


def _valid(lengths, B, T):
    """(B, T) bool: t < lengths[b] (all true without lengths)."""
    if lengths is None:
        return np.ones((B, T), bool)
    return np.arange(T)[None, :] < np.asarray(lengths)[:, None]


def forward(dtype, Wx, scale, shift, alpha, u0, mode, lengths=None, class_order=None):
    assert mode in MODES
    U, _ = sn.readout_forward(dtype, Wx, scale, shift, alpha, u0, class_order)
    B, T, C = U.shape
    m = _valid(lengths, B, T)
    p = np.where(m[:, :, None], sn._softmax(U, class_order), dtype(0))
    acc = np.zeros((B, C), dtype)
    run = np.empty((B, T, C), dtype)
    for t in range(T):                      # the one sequential sum that makes `out`
        acc = acc + p[:, t]
        run[:, t] = acc
    seq = p if mode == "prob" else np.where(m[:, :, None], run, dtype(0))
    return {"u_save": U, "out": acc, "seq": seq}


def reverse_running_sum(g_seq, dtype=F32, lengths=None):
    g = np.asarray(g_seq)
    B, T, C = g.shape
    m = _valid(lengths, B, T)
    g = np.where(m[:, :, None], g, 0).astype(dtype)
    S = np.zeros((B, C), dtype)
    out = np.zeros((B, T, C), dtype)
    for t in range(T - 1, -1, -1):
        S = S + g[:, t]
        out[:, t] = S
    return np.where(m[:, :, None], out, dtype(0))


def backward(dtype, g_out, g_seq, mode, u_save, alpha, u0, bn=None, lengths=None, class_order=None):
    assert mode in MODES
    B, T, C = np.asarray(u_save).shape
    m = _valid(lengths, B, T)[:, :, None]
    U = np.where(m, np.asarray(u_save), 0).astype(dtype)
    g = np.zeros((B, C), dtype) if g_out is None else np.asarray(g_out, dtype=dtype)
    A = (np.where(m, np.asarray(g_seq), 0).astype(dtype) if mode == "prob"
         else reverse_running_sum(g_seq, dtype, lengths))
    G = g[:, None, :] + A
    raw = np.asarray(alpha, dtype=F32)
    lo, hi = sn.LIMS["alpha"]
    al = np.minimum(np.maximum(raw.astype(dtype), dtype(lo)), dtype(hi))
    oma = dtype(1) - al
    p = sn._softmax(U, class_order)
    dot = sn.ordered_sum(p * G, -1, class_order)
    e = np.where(m, p * (G - dot[..., None]), dtype(0))
    du, acc = np.zeros((B, C), dtype), np.zeros((B, C), dtype)
    dWx = np.empty((B, T, C), dtype)
    for t in range(T - 1, -1, -1):          # (tests/spiking_numpy.py readout_backward's loop, e per step)
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
    """(out, seq) in Wx's dtype, differentiable."""
    assert mode in MODES
    B, T, C = Wx.shape
    lo, hi = (float(v) for v in sn.LIMS["alpha"])
    al = torch.clamp(alpha, min=lo, max=hi)
    valid = torch.from_numpy(_valid(lengths, B, T)).to(Wx.dtype)
    u, out, rows = u0, torch.zeros(B, C, dtype=Wx.dtype), []
    for t in range(T):
        u = al * u + (1 - al) * Wx[:, t, :]
        p = torch.softmax(u, dim=1) * valid[:, t, None]
        out = out + p
        rows.append(p if mode == "prob" else out * valid[:, t, None])
    return out, torch.stack(rows, dim=1)


def check_against_oracle(B=3, T=11, C=5, seed=0):
    """The anchor of this file on oracle.bptt_numpy (module docstring).  Returns the worst relative difference seen."""
    rng = np.random.default_rng(seed)
    Wx = rng.standard_normal((B, T, C)).astype(F32)
    alpha = rng.uniform(0.83, 0.95, C).astype(F32)
    alpha[0] = 0.5
    u0 = rng.uniform(0, 1, (B, C)).astype(F32)
    g = rng.standard_normal((B, C)).astype(F32)
    out_o, U_o = bptt.readout_forward(Wx, alpha, u0)
    worst = 0.0
    for mode in MODES:
        f = forward(F32, Wx, None, None, alpha, u0, mode)
        assert np.array_equal(f["u_save"], U_o)
        np.testing.assert_allclose(f["out"], out_o, rtol=1e-6)
        b = backward(F32, g, np.zeros((B, T, C), F32), mode, U_o, alpha, u0)
        ref = bptt.readout_backward(g, Wx, alpha, u0, U_o)
        for k in ("dWx", "alpha"):
            key = "dalpha" if k == "alpha" else k
            worst = max(worst, float(np.abs(b[k] - ref[key]).max() / np.abs(ref[key]).max()))
    # "sum": row t is the sequential fp32 sum over the prefix — the oracle's `out` of the first t + 1 steps.  The oracle
    # takes its softmax denominator with numpy's sum, so the restatement runs with class_order None here.
    f = forward(F32, Wx, None, None, alpha, u0, "sum")
    for t in range(T):
        out_t, _ = bptt.readout_forward(Wx[:, :t + 1], alpha, u0)
        np.testing.assert_allclose(f["seq"][:, t], out_t, rtol=3e-7, atol=0)
    assert np.array_equal(f["seq"][:, -1], f["out"])
    return worst
