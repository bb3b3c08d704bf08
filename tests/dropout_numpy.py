"""
TEST INFRASTRUCTURE ONLY: the in-kernel dropout mask restated in plain numpy.

Contract (include/sparch_hip.h, "Dropout"; arithmetic in sparch_amd/csrc/common.h): nothing is stored, forward
and backward each regenerate

    keep(seed, idx) = uniform(hash(seed, idx)) >= p,      kept values scale by fp32(1 / (1 - p))

from the 64-bit seed of the launch and the 64-bit index of the OUTPUT element in the layer's contiguous
(B, T, F) result — F the width the kernel runs at: H * dirs, and the PADDED width where a layer runs padded
(a recurrent spiking layer with H % 4 != 0 runs at H4 = 4 * ceil(H / 4) per direction; its mask is
`keep_mask(seed, (B, T, dirs * H4), p).reshape(B, T, dirs, H4)[..., :H].reshape(B, T, dirs * H)`, see
`keep_mask_padded`).

The hash is two rounds of the lowbias32 integer finaliser, all in uint32 with wrap-around:

    a = mix32(lo(idx) ^ lo(seed))
    b = mix32(a + hi(idx) * 0x9E3779B9 + hi(seed))
    u = fp32(b >> 8) * 2^-24            (24 bits: exact in fp32)
    keep iff u >= fp32(p)               (compared in fp32)

This file restates the documented contract and shares no code with the product; the GPU tests pin it to the
kernels through what a forward shows (every non-zero undropped output equals raw * mask there).
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def _mix32(x):
    """lowbias32 on uint32 values carried in uint64 arrays (products masked back to 32 bits)."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def uniforms(seed, n, first_index=0):
    """The 24-bit uniforms in [0, 1) of elements first_index .. first_index + n - 1, float32."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    first_index = int(first_index)
    assert 0 <= first_index and first_index + n <= 1 << 64
    idx = np.arange(n, dtype=np.uint64) + np.uint64(first_index)
    s_lo, s_hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    a = _mix32((idx & _M32) ^ s_lo)
    b = _mix32((a + (idx >> np.uint64(32)) * np.uint64(0x9E3779B9) + s_hi) & _M32)
    return (b >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def inv_keep(p):
    """fp32(1) / (fp32(1) - fp32(p)), as the entry points compute it."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_mask(seed, shape, p, first_index=0):
    """float32 array of `shape` (C order = the kernel's element index): 0 where dropped, fp32(1/(1-p)) where kept."""
    n = int(np.prod(shape))
    u = uniforms(seed, n, first_index)
    return np.where(u >= np.float32(p), inv_keep(p), np.float32(0.0)).astype(np.float32).reshape(shape)


def keep_mask_padded(seed, B, T, dirs, H, Hp, p):
    """Mask of a layer that runs at the padded width Hp >= H per direction, sliced to the caller's (B, T, dirs * H)."""
    m = keep_mask(seed, (B, T, dirs, Hp), p)
    return np.ascontiguousarray(m[..., :H]).reshape(B, T, dirs * H)
