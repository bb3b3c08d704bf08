"""
The data movements of csrc/bidir.hip restated with NumPy indexing (tests/test_bidir_kernels_gpu.py,
tests/test_bidir_ragged_host.py), written independently of the kernels and of sparch_amd.snns.prepare_bidir_packing.

The doubled batch of a bidirectional layer on B clips has 2B rows: row b is clip b, row B + b is clip b read backwards
inside its own length.  The packed forms are the padded ones under tests/packed_numpy.py: the single tensors packed by
the lengths, the doubled ones by the lengths twice (the doubled plan follows prepare_packing's own rules).
"""
import numpy as np

from tests import packed_numpy as pn


def split(x, lengths):
    """x (B,T,...) -> (2B,T,...): the rows, then every row flipped inside its length; zeros on all tails."""
    B = x.shape[0]
    out = np.zeros((2 * B,) + x.shape[1:], x.dtype)
    for b, L in enumerate(lengths):
        out[b, :L] = x[b, :L]
        out[B + b, :L] = x[b, :L][::-1]
    return out


def split_bwd(g, lengths):
    """g (2B,T,C) float32 -> (B,T,C): g[b,t] + g[B+b, L-1-t] (one float32 sum), zero on the tails."""
    B = g.shape[0] // 2
    out = np.zeros((B,) + g.shape[1:], np.float32)
    for b, L in enumerate(lengths):
        out[b, :L] = g[b, :L] + g[B + b, :L][::-1]
    return out


def join(s, lengths):
    """s (2B,T,H) -> (B,T,2H): forward columns first, the reverse rows back in the clip's own order; zero tails."""
    B, T, H = s.shape[0] // 2, s.shape[1], s.shape[2]
    out = np.zeros((B, T, 2 * H), s.dtype)
    for b, L in enumerate(lengths):
        out[b, :L, :H] = s[b, :L]
        out[b, :L, H:] = s[B + b, :L][::-1]
    return out


def join_bwd(g, g_rate, rate_scale, lengths):
    """g (B,T,2H) float32 -> (2B,T,H): the gather, plus g_rate[column] * rate_scale (a float32 product, then a float32
    sum) on the valid steps; zero tails."""
    B, T, H = g.shape[0], g.shape[1], g.shape[2] // 2
    r = np.zeros(2 * H, np.float32) if g_rate is None else (g_rate.astype(np.float32) * np.float32(rate_scale))
    out = np.zeros((2 * B, T, H), np.float32)
    for b, L in enumerate(lengths):
        v = g[b, :L] + r[None, :] if g_rate is not None else g[b, :L]
        out[b, :L] = v[:, :H]
        out[B + b, :L] = v[:, H:][::-1]
    return out.astype(np.float32)


def doubled_plan(lengths):
    """(order2, lens2, offsets2 (2B + 1,), inverse2, fwd (B,), rev (B,)): packed_numpy.plan_of on the lengths twice, and
    per sequence j of the SINGLE plan the first doubled row of its forward and of its reversed copy."""
    lengths = np.asarray(lengths, np.int64)
    B = len(lengths)
    order, _, _, _ = pn.plan_of(lengths)
    order2, lens2, offsets2, _ = pn.plan_of(np.concatenate([lengths, lengths]))
    inverse2 = np.empty(2 * B, np.int64)
    for j, b in enumerate(order2):
        inverse2[b] = j
    fwd = np.asarray([offsets2[inverse2[b]] for b in order], np.int64)
    rev = np.asarray([offsets2[inverse2[B + b]] for b in order], np.int64)
    return order2, lens2, offsets2, inverse2, fwd, rev


def pack2(x2, lengths):
    """A doubled padded tensor (2B,T,...) -> its packed form (2N,...)."""
    return pn.pack(x2, list(lengths) + list(lengths))
