"""
Shared cases of the SHD / SSC event tests: a small file as a mapping, the hand-made samples of the gather-and-bin kernel,
the resident store made of them and a batch as a dense tensor.  sparch_amd is imported only inside functions.
"""
import numpy as np

from tests.kit import DEV


def fake_h5(n=11, seed=3, tdtype=np.float32):
    """An SHD / SSC file as a mapping: sorted times in `tdtype`, one empty sample, events exactly on the first edge."""
    rng = np.random.default_rng(seed)
    times, units = [], []
    for i in range(n):
        m = int(rng.integers(0, 400)) if i != 4 else 0
        t = np.sort(rng.uniform(0.0, 1.39, m)).astype(tdtype)
        if m > 3:
            t[:2] = 0.0
        times.append(t)
        units.append(rng.integers(0, 700, m).astype(np.int32))
    return {"spikes": {"times": times, "units": units}, "labels": rng.integers(0, 20, n)}


def samples(rng, nb_steps, nb_units, max_time, tdtype, n_random, sort):
    """(times, units) per sample: an empty one, random ones of up to a few thousand events, and one of hand-made
    cases — events exactly on edges, duplicates, t < 0, t >= max_time, units out of range."""
    edges = np.linspace(0, max_time, nb_steps)
    out = [(np.zeros(0, tdtype), np.zeros(0, np.int64))]
    for i in range(n_random):
        m = int(rng.integers(1, 6000 if i % 3 == 0 else 300))
        out.append((rng.uniform(0, max_time, m).astype(tdtype), rng.integers(0, nb_units, m)))
    on_edge = edges[[0, 1, nb_steps // 2, nb_steps - 1]].astype(tdtype)           # rounded to the store's format
    below = np.nextafter(on_edge[1:2], tdtype(0))
    t = np.concatenate([on_edge, below, np.array([0.7, 0.7, 0.7, 0.7, -0.1, -1e-3, max_time, 1.5 * max_time, 9.0,
                                                  0.3, 0.31, 0.32], np.float64).astype(tdtype)])
    u = np.concatenate([np.arange(len(on_edge) + 1) % nb_units,
                        np.array([0, 0, 0, nb_units - 1, 0, nb_units - 1, 0, 0, 0, nb_units, -1, 70000])])
    out.append((t, u))
    out.append((np.zeros(0, tdtype), np.zeros(0, np.int64)))                        # the last sample is empty too
    if sort:
        out = [(t[o], u[o]) for t, u in out for o in [np.argsort(t, kind="stable")]]
    else:
        out = [(t[o], u[o]) for t, u in out for o in [rng.permutation(len(t))]]
    return out


def store(samples, nb_units, max_time, labels=None):
    from sparch_amd import functional as Fn

    labels = np.arange(len(samples)) * 3 if labels is None else labels
    h5 = {"spikes": {"times": [s[0] for s in samples], "units": [s[1] for s in samples]}, "labels": labels}
    return Fn.EventStore.from_mapping(h5, device=DEV, nb_units=nb_units, max_time=max_time)


def dense(x):
    from sparch_amd import functional as Fn

    tag = Fn.input_plane_of(x)
    if tag is None:
        return x
    B, T, K = x.shape
    return tag[0].view(B, T, -1)[:, :, :K].float()
