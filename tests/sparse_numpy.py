"""NumPy restatement of the event-driven streaming step's summation order (csrc/streamsparse.hip) — test helper.

A row's non-zero inputs are listed in ascending position; entry p of the list goes to partial sum p mod `ways`, each an
fp32 FMA chain acc = fma(value, wt, acc) in ascending p; the partial sums are added pairwise in one fixed tree,
(p0 + p1) + (p2 + p3) for the hidden layers' ways = 4.  The readout runs ONE chain per class (ways = 1).  An fma is
computed as the fp64 product (exact: two 24-bit significands) plus the accumulator in fp64, rounded to fp32.
"""
import numpy as np

f32 = np.float32


def active_list(row):
    """The compacted (k, value) pairs of one row: positions of the non-zero values, ascending, and the values."""
    row = np.asarray(row, dtype=f32)
    k = np.flatnonzero(row != 0)
    return k, row[k]


def sparse_dot(X, Wt, ways=4):
    """X (B,K) times Wt (K,H) in the kernel's documented order, fp32 (B,H)."""
    X, Wt = np.asarray(X, dtype=f32), np.asarray(Wt, dtype=f32)
    assert X.ndim == 2 and Wt.ndim == 2 and X.shape[1] == Wt.shape[0] and ways in (1, 2, 4)
    Wd = Wt.astype(np.float64)
    out = np.zeros((X.shape[0], Wt.shape[1]), f32)
    for b in range(X.shape[0]):
        ks, vs = active_list(X[b])
        acc = np.zeros((ways, Wt.shape[1]), f32)
        for p, (k, v) in enumerate(zip(ks, vs)):
            w = p % ways
            acc[w] = (np.float64(v) * Wd[k] + acc[w].astype(np.float64)).astype(f32)
        parts = list(acc)
        while len(parts) > 1:
            parts = [parts[i] + parts[i + 1] for i in range(0, len(parts), 2)]
        out[b] = parts[0]
    return out
