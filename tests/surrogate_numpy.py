"""
TEST INFRASTRUCTURE ONLY: the reverse pass of tests/spiking_numpy.backward with the surrogate gradient's gate as a
parameter.  Plain numpy, generic in dtype, no code shared with the product.  Every other convention is
spiking_numpy's, by import: the geometry and layouts, the clamped Params, the decisions taken on the difference in the
save's own type, `k_order` / `row_order`, `keep`, `bn`, `operand` / `rec_operand`, and the returned dict.

With x = u_t - theta, the difference in the SAVE's own type (fp32 from a kernel: the value its spike decision uses),
widened to `dtype` before the gate's arithmetic, ds the gradient reaching the spike and k > 0 a scale:

    boxcar        ds where -0.5 < x <= 0.5, else 0 (assignment; takes no scale)         area 1
    triangle      ds * max(0, 1 - k*abs(x))                                              area 1/k
    fast_sigmoid  ds / ((1 + k*abs(x)) * (1 + k*abs(x)))                                 area 2/k
    atan          ds / (1 + (k*x)*(k*x))                                                 area pi/k

in exactly that operation order (one rounding per operation in `dtype`, as the kernels' -ffp-contract=off arithmetic).

du_t = gate(ds_t, x_t) + alpha du_{t+1} [+ a dw_{t+1}]; everything else of the pass is spiking_numpy's docstring.

MUTANTS (tests/test_surrogate_host.py only, the sharpness of the GPU file's bound):
    "scale_ignored"   k = 1
    "abs_dropped"     abs(x) replaced by x; for atan, which has no abs, x shifted by 0.125
    "boxcar"          the box-car in place of the smooth gate
    "square_dropped"  fast_sigmoid: ds / (1 + k*abs(x)); atan: ds / (1 + abs(k*x)); the triangle has no square
"""
import math

import numpy as np

from tests import spiking_numpy as sn

SURROGATES = ("boxcar", "triangle", "fast_sigmoid", "atan")
SMOOTH = SURROGATES[1:]
IDS = {name: i for i, name in enumerate(SURROGATES)}                      # SPARCH_SURROGATE_*
DEFAULT_SCALE = {"triangle": 1.0, "fast_sigmoid": 2.0, "atan": math.pi}    # the gate's area is then the box-car's: 1
AREA = {"boxcar": lambda k: 1.0, "triangle": lambda k: 1.0 / k, "fast_sigmoid": lambda k: 2.0 / k,
        "atan": lambda k: math.pi / k}
TEST_SCALE = {"triangle": 2.0, "fast_sigmoid": 5.0, "atan": 2.5}           # the scales of the sharpness and GPU cases
MUTANTS = ("scale_ignored", "abs_dropped", "boxcar", "square_dropped")


def mutants_of(name):
    return tuple(m for m in MUTANTS if not (m == "square_dropped" and name == "triangle"))


def gate(name, k, ds, x, mutant=None):
    """gate(ds, x) in ds's dtype; x already in that dtype."""
    assert name in SURROGATES and (mutant is None or mutant in MUTANTS), (name, mutant)
    dt = ds.dtype.type
    if name == "boxcar" or mutant == "boxcar":
        return np.where((x <= dt(-0.5)) | (x > dt(0.5)), dt(0), ds)
    k = dt(1) if mutant == "scale_ignored" else dt(k)
    if name == "atan":
        kx = k * (x + dt(0.125) if mutant == "abs_dropped" else x)
        return ds / (dt(1) + (np.abs(kx) if mutant == "square_dropped" else kx * kx))
    ax = x if mutant == "abs_dropped" else np.abs(x)
    if name == "triangle":
        return ds * np.maximum(dt(0), dt(1) - k * ax)
    d = dt(1) + k * ax
    return ds / (d if mutant == "square_dropped" else d * d)


def backward(kind, dtype, g_out, g_rate, u_save, w_save, p, u0, w0, s0, *, B, dirs, surrogate=("boxcar", None), theta=1.0,
             k_order=None, operand=None, rec_operand=None, bn=None, keep=None, row_order=None, mutant=None):
    """spiking_numpy.backward's reverse recurrences on supplied saves with gate `surrogate` = (name, scale).  Same
    arguments (without its own mutants and rec_product) and the same returned dict."""
    name, scale = surrogate
    P = sn.Params(kind, dtype, p, theta, operand)
    Bp, T, H = u_save.shape
    go = np.asarray(g_out, dtype=dtype)
    if g_rate is not None:
        go = go + (np.asarray(g_rate, dtype=dtype) * (dtype(1) / (dtype(B) * dtype(T))))[None, None, :]
    if keep is not None:
        go = go * np.asarray(keep, dtype=dtype)
    g = sn.from_out_layout(go, dirs)
    us = np.asarray(u_save)
    U = us.astype(dtype)
    XS = us - us.dtype.type(theta)                     # in the save's own type: the spike's difference
    S = (XS > 0).astype(dtype)
    X = XS.astype(dtype)
    W = np.asarray(w_save, dtype=dtype) if P.adaptive else None
    u0, s0 = np.asarray(u0, dtype=dtype), np.asarray(s0, dtype=dtype)
    w0 = np.asarray(w0, dtype=dtype) if P.adaptive else None
    rec_op = None if rec_operand is None else sn.to_original(np.asarray(rec_operand, dtype=dtype), B, dirs)
    du_n, dw_n = np.zeros((Bp, H), dtype), np.zeros((Bp, H), dtype)
    dWx = np.empty((Bp, T, H), dtype)
    acc = {k: np.zeros((Bp, H), dtype) for k in ("alpha", "beta", "a", "b")}
    dV = np.zeros((H, H), dtype) if P.recurrent else None
    dwx_next = None
    for t in range(T - 1, -1, -1):
        u_prev, s_prev = (U[:, t - 1], S[:, t - 1]) if t > 0 else (u0, s0)
        aldu = P.alpha * du_n
        ds = g[:, t] - aldu
        if P.adaptive:
            ds = ds + P.b * dw_n
        if P.recurrent and t + 1 < T:
            x_op = P.op(dwx_next if rec_op is None else rec_op[:, t + 1])
            ds = ds + sn.matmul_blocks(x_op, P.VmT, k_order)
        du = gate(name, scale, ds, X[:, t], mutant) + aldu
        if P.adaptive:
            du = du + P.a * dw_n
        dwx = P.oma * du
        dWx[:, t] = dwx
        acc["alpha"] = acc["alpha"] + du * ((u_prev - s_prev) - U[:, t])
        if P.adaptive:
            dw = P.beta * dw_n - dwx
            acc["beta"] = acc["beta"] + dw * (W[:, t - 1] if t > 0 else w0)
            acc["a"] = acc["a"] + dw * u_prev
            acc["b"] = acc["b"] + dw * s_prev
            dw_n = dw
        if P.recurrent:
            x_op = P.op(dwx if rec_op is None else rec_op[:, t])
            dV = dV + (P.op(s_prev) if t == 0 else s_prev).T @ x_op
        du_n, dwx_next = du, dwx
    acc["alpha"] = acc["alpha"] / P.oma
    out = {"dWx": sn.to_original(dWx, B, dirs)}
    for k in ("alpha",) + (("beta", "a", "b") if P.adaptive else ()):
        out["ws_" + k] = acc[k]
        out[k] = np.where(sn.inside(P.raw[k], sn.LIMS[k]), sn.ordered_sum(acc[k], 0, row_order), dtype(0))
    if P.recurrent:
        np.fill_diagonal(dV, 0)
        out["V"] = dV
    if bn is not None:
        x_raw, mean, invstd = (np.asarray(v, dtype=dtype) for v in bn)
        xhat = (x_raw - mean) * invstd
        dy = out["dWx"].reshape(dirs, B, T, H)
        if row_order is None:
            out["bn_sums"] = (dy.sum((0, 1, 2)), (dy * xhat[None]).sum((0, 1, 2)))
        else:       # per virtual row over its steps in reverse cell time, then over the rows
            rev = lambda q: sn.to_original(q.reshape(Bp, T, H), B, dirs)[:, ::-1]  # noqa: E731
            out["bn_sums"] = tuple(sn.ordered_sum(sn.ordered_sum(rev(q), 1, "asc"), 0, row_order)
                                   for q in (dy, dy * xhat[None]))
    return out
