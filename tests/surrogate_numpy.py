"""
TEST INFRASTRUCTURE ONLY: the gates of the surrogate gradient, and the reverse pass with one of them: backward() here
is tests/spiking_numpy.backward(gate=...), the ONE statement of the reverse recurrences.  Plain numpy, generic in dtype,
no code shared with the product.  Everything but the gate is spiking_numpy's: the geometry and layouts, the clamped
Params, the decisions taken on the difference in the save's own type, `k_order` / `row_order`, `keep`, `bn`, `operand`
/ `rec_operand`, and the returned dict.

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
import functools
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
    return sn.backward(kind, dtype, g_out, g_rate, u_save, w_save, p, u0, w0, s0, B=B, dirs=dirs, theta=theta,
                       k_order=k_order, operand=operand, rec_operand=rec_operand, bn=bn, keep=keep, row_order=row_order,
                       gate=functools.partial(gate, name, scale, mutant=mutant))
