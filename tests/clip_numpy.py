"""
TEST INFRASTRUCTURE ONLY: gradient clipping by global norm (sparch_amd/csrc/gradclip.hip, sparch_adam_step_clip in
sparch_amd/csrc/optim.hip) restated in plain numpy.  It shares no code with the product.

  norm_ref(tensors)            the 2-norm over a list of fp32 arrays in float64 (None / empty entries add nothing)
  coef_f32(norm32, max_norm)   the kernel's three fp32 operations on an fp32 norm: norm + 1e-6f, max_norm / that,
                               min(that, 1) — torch.nn.utils.clip_grad_norm_'s formula and epsilon
  coef_ref(norm, max_norm)     the same formula in float64
  clip_table(n_tensors, ...)   the tensor tables of tests/test_gradclip_gpu.py

The bound of the norm, NORM_U = 2 u relative (u = 2^-24) + TINY, is derived, not calibrated: the kernels accumulate
(double)g * g in double — every product of two fp32 values is EXACT in double, a sum of n <= 2^27 terms is off by at
most n * 2^-53 < u / 4 relative whatever the order — take the square root in double (half of that error, plus 2^-53)
and round to fp32 ONCE (at most u relative to the result).  2 u covers it with room; nothing here was fitted to a
kernel.
"""
import numpy as np

from tests import head_numpy as hn
from tests.kit import F32, F64

U = 2.0 ** -24
TINY = 2.0 ** -126
NORM_U = 2.0 * U


def norm_ref(tensors):
    """float64 2-norm of the fp32 values of every array in `tensors` (None: an empty tensor)."""
    total = 0.0
    for t in tensors:
        if t is not None and np.size(t):
            a = np.asarray(t, dtype=F32).astype(F64).ravel()
            total += float(np.dot(a, a))
    return float(np.sqrt(total))


def coef_ref(norm, max_norm):
    return min(float(max_norm) / (float(norm) + 1e-6), 1.0)


def coef_f32(norm32, max_norm):
    """The kernel's coefficient from ITS fp32 norm: three fp32 operations, each correctly rounded."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        d = F32(norm32) + F32(1e-6)
        q = F32(max_norm) / d
        return F32(np.fmin(q, F32(1.0)))


def table_sizes(n_tensors):
    """ADAM_SIZES repeated to n_tensors entries; a repeated table has two empty tensors in its middle."""
    sizes = [hn.ADAM_SIZES[i % len(hn.ADAM_SIZES)] for i in range(n_tensors)]
    if n_tensors > len(hn.ADAM_SIZES):
        sizes[n_tensors // 2 - 1] = 0
        sizes[n_tensors // 2] = 0
    return sizes


def clip_table(n_tensors, t=2, weight_decay=0.0, seed=0, fill=None):
    """One (p, g, m, v) of fp32 arrays per tensor (None for an empty one), values from head_numpy.adam_inputs (five
    gradient scales from 1e-12 to 1e12 side by side).  fill: every gradient element is this value instead."""
    out = []
    for i, n in enumerate(table_sizes(n_tensors)):
        if n == 0:
            out.append(None)
            continue
        # (element 0 of adam_inputs has g = m = v = 0: drawn one longer and dropped, as tests/test_head_kernels_gpu.py)
        p, g, m, v = (a[1:] for a in hn.adam_inputs(n + 1, t, weight_decay, seed + 31 * i))
        if fill is not None:
            g = np.full(n, fill, dtype=F32)
        out.append((p, g, m, v))
    return out


def unaligned_slot(table):
    """The tensor of a table whose gradient the GPU tests place at element offset 1 of a larger buffer: the first one of
    4097 elements (two workgroups, a ragged tail)."""
    return next(i for i, h in enumerate(table) if h is not None and h[1].size == 4097)
