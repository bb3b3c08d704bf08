"""
Packed ragged batches restated in numpy (tests/test_packed_host.py, tests/test_packed_gpu.py): the plan — stable descending
order, sorted lengths, exclusive prefix sum — and the row gather / scatter of csrc/pack.hip, written independently of
sparch_amd.snns.prepare_packing and of the kernels.
"""
import numpy as np


def plan_of(lengths):
    """lengths (B,) -> (order, sorted lengths, offsets (B + 1,), N): sequence j of the order is batch row order[j]; ties
    keep the batch order (a stable sort); offsets is the exclusive prefix sum and offsets[B] = N."""
    lengths = np.asarray(lengths, np.int64)
    order = np.asarray(sorted(range(len(lengths)), key=lambda b: (-int(lengths[b]), b)), np.int64)
    lens = lengths[order]
    offsets = np.zeros(len(lengths) + 1, np.int64)
    for j, n in enumerate(lens):
        offsets[j + 1] = offsets[j] + n
    return order, lens, offsets, int(offsets[-1])


def pack(x, lengths):
    """x (B,T,C) -> (N,C): step t < lengths[order[j]] of batch row order[j] at packed row offsets[j] + t."""
    order, lens, offsets, n = plan_of(lengths)
    out = np.empty((n,) + x.shape[2:], x.dtype)
    for j, b in enumerate(order):
        for t in range(int(lens[j])):
            out[offsets[j] + t] = x[b, t]
    return out


def unpack(xp, lengths, T):
    """xp (N,C) -> (B,T,C) in the batch's own row order, zeros on every row's steps t >= lengths[b]."""
    order, lens, offsets, n = plan_of(lengths)
    assert xp.shape[0] == n
    out = np.zeros((len(order), T) + xp.shape[1:], xp.dtype)
    for j, b in enumerate(order):
        out[b, :lens[j]] = xp[offsets[j]:offsets[j] + lens[j]]
    return out


def unpack_sorted(xp, lens, T):
    """The same for rows that are already in packed order (order = identity): (B,T,C) with zero tails."""
    lens = np.asarray(lens, np.int64)
    assert (np.diff(lens) <= 0).all()
    return unpack(xp, lens, T)


def valid_mask(lengths, T):
    return np.arange(T)[None, :] < np.asarray(lengths)[:, None]


def packed_index(lengths, T, width):
    """(B,T,width) int64: the element index in the packed (N,width) tensor of every valid (b, t, h) — what the packed
    kernels hash for their dropout masks — and -1 on the padding."""
    order, lens, offsets, _ = plan_of(lengths)
    idx = -np.ones((len(order), T, width), np.int64)
    for j, b in enumerate(order):
        rows = offsets[j] + np.arange(int(lens[j]))
        idx[b, :lens[j]] = rows[:, None] * width + np.arange(width)[None, :]
    return idx
